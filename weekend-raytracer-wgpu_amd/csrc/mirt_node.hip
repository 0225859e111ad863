// mirt_node.hip — the node of include/mirt.h (mirt_node_*): ONE host process renders one frame on N member contexts, one per
// entry of a device list.  Member i renders its share of the 4-row tile interleave (tile_rows = 4, n_parts = N, part = i, the
// partition multi_gpu.py uses); the parts come to member 0 and assemble_parts_kernel (mirt_kernels.hip) writes the band there.
//
// Transports
//   loopback (every entry names one device): the members' parts stay in their own buffers; the assembly reads them in place.
//   RCCL (all entries distinct, or MIRT_NODE_RCCL): one ncclGather per member inside ncclGroupStart/End, on the member streams,
//        into a parts buffer on member 0 (every part padded to the largest).  librccl is loaded with dlopen by such a node only.
//
// Ordering (no host sync on the frame path)
//   member i:  [wait ev_consumed] fill part i on its context stream -> ev_done[i]
//              (fill = mirt_ctx_render_device, or mirt_ctx_accum_frame_device for a progressive frame: the ONLY difference between the two)
//   loopback:  tail stream waits ev_done[i] of every member with rows
//   RCCL:      member 0's stream waits ev_done[i > 0] -> ev_gather_begin -> group of gathers -> ev_gather_end; tail waits ev_gather_end
//   tail:      assemble_parts_kernel (events ev_asm_begin / ev_asm_end on its dispatch) -> ev_consumed [-> D2H copy]
// The tail stream is the caller's stream (mirt_node_render_device) or the node's own stream on member 0's device.  No event is
// recorded on, or waited for from, hipStreamLegacy: that stream is refused.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types only: the functions come from dlsym

#include <dlfcn.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mirt.h"
#include "mirt_kernels.h"

namespace {

constexpr uint32_t kNodeTileRows = 4;      // the interleave of multi_gpu.py (DEFAULT_TILE_ROWS)
static_assert(MIRT_NODE_MAX_MEMBERS <= mirt::kAssembleMaxParts, "the assembly kernel's pointer table holds every member's part");

#define NODE_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return mirt::set_error(MIRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- librccl through dlopen ----
struct Rccl {
    decltype(&ncclCommInitAll)    comm_init_all = nullptr;
    decltype(&ncclCommDestroy)    comm_destroy = nullptr;
    decltype(&ncclGather)         gather = nullptr;
    decltype(&ncclGroupStart)     group_start = nullptr;
    decltype(&ncclGroupEnd)       group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};

// The process's librccl: one already loaded (torch brings its own) first, else ROCm's.  nullptr (and the message) if neither.
const Rccl* load_rccl()
{
    static std::mutex mu;
    static Rccl r;
    static bool loaded = false;
    std::lock_guard<std::mutex> lock(mu);
    if (loaded) return &r;
    void* h = nullptr;
    for (const char* name : { "librccl.so", "librccl.so.1" })
        if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    if (!h) {
        const char* rocm = std::getenv("ROCM_PATH");
        const std::string path = std::string(rocm && *rocm ? rocm : "/opt/rocm") + "/lib/librccl.so.1";
        h = dlopen(path.c_str(), RTLD_NOW);
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
    if (!h) {
        const char* why = dlerror();
        mirt::set_error(MIRT_ERR_HIP, "RCCL: librccl could not be loaded (%s)", why ? why : "not found");
        return nullptr;
    }
    Rccl t;
    t.comm_init_all = reinterpret_cast<decltype(t.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
    t.comm_destroy = reinterpret_cast<decltype(t.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    t.gather = reinterpret_cast<decltype(t.gather)>(dlsym(h, "ncclGather"));
    t.group_start = reinterpret_cast<decltype(t.group_start)>(dlsym(h, "ncclGroupStart"));
    t.group_end = reinterpret_cast<decltype(t.group_end)>(dlsym(h, "ncclGroupEnd"));
    t.error_string = reinterpret_cast<decltype(t.error_string)>(dlsym(h, "ncclGetErrorString"));
    if (!t.comm_init_all || !t.comm_destroy || !t.gather || !t.group_start || !t.group_end || !t.error_string) {
        mirt::set_error(MIRT_ERR_HIP, "RCCL: the loaded librccl lacks ncclGather / ncclCommInitAll / ncclGroupStart");
        return nullptr;
    }
    r = t;
    loaded = true;
    return &r;
}

template <typename T>
int grow(T** ptr, size_t* cap, size_t need)       // device buffer of at least `need` elements on the current device; never shrinks
{
    if (need <= *cap && *ptr) return MIRT_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    const size_t bytes = (need ? need : 1) * sizeof(T);
    if (hipMalloc(ptr, bytes) != hipSuccess) return mirt::set_error(MIRT_ERR_ALLOC, "hipMalloc(%zu bytes) failed", bytes);
    *cap = need ? need : 1;
    return MIRT_OK;
}

}  // namespace

struct MirtNode {
    uint32_t     n = 0;
    uint32_t     transport = 0;                                 // 0 loopback, 1 RCCL
    int          device[MIRT_NODE_MAX_MEMBERS] = {};
    MirtContext* ctx[MIRT_NODE_MAX_MEMBERS] = {};
    hipStream_t  stream[MIRT_NODE_MAX_MEMBERS] = {};            // member i's own context stream (mirt_ctx_frame_stream 0): it renders there
    hipEvent_t   ev_done[MIRT_NODE_MAX_MEMBERS] = {};           // member i's part is rendered
    uint32_t*    d_part[MIRT_NODE_MAX_MEMBERS] = {};            // member i's compact part (RCCL: its send buffer, padded to the largest part)
    size_t       cap_part[MIRT_NODE_MAX_MEMBERS] = {};          // pixels
    ncclComm_t   comm[MIRT_NODE_MAX_MEMBERS] = {};
    const Rccl*  rccl = nullptr;
    hipStream_t  root_stream = nullptr;                         // the node's own stream on member 0's device
    hipEvent_t   ev_consumed = nullptr;                         // the last assembly has read the parts
    bool         consumed_pending = false;
    hipEvent_t   ev_asm_begin = nullptr, ev_asm_end = nullptr;  // timing of the last assembly kernel (on its dispatch)
    bool         asm_timed = false;
    hipEvent_t   ev_gather_begin = nullptr, ev_gather_end = nullptr;   // RCCL, on member 0's stream
    bool         gather_timed = false;
    uint32_t*    d_gather = nullptr;                            // RCCL: n slots of the largest part, on member 0
    size_t       cap_gather = 0;
    uint32_t*    d_out = nullptr;                               // mirt_node_render: the band before its D2H copy
    size_t       cap_out = 0;
    bool         have_scene = false;
    // progressive accumulation: member i owns the exact sums of its part (mirt_ctx_accum_reset with q[i]); what crosses devices per frame
    // is the members' RGBA8 parts, never the sums
    bool         accum_valid = false;                           // a reset succeeded and no member's frame has failed since
    MirtParams   accum_params = {};                             // the reset's params (geometry of the sums)
    uint32_t     accum_samples = 0;
};

namespace {

// What fills member i's part: a one-shot render, or one progressive frame on the member's own sums.
enum Fill { kFillRender, kFillAccumFrame };

int fill_part(Fill fill, MirtContext* ctx, const MirtParams* q, void* d_part, size_t len, void* stream)
{
    return fill == kFillRender ? mirt_ctx_render_device(ctx, q, d_part, len, stream) : mirt_ctx_accum_frame_device(ctx, q, d_part, len, stream);
}

// Member i's share of the band: the 4-row tile interleave.  Returns the largest number of rows a member has.
uint32_t member_params(const MirtNode* nd, const MirtParams* p, MirtParams* q, uint32_t* rows)
{
    uint32_t max_rows = 0;
    for (uint32_t i = 0; i < nd->n; ++i) {
        q[i] = *p;
        q[i].tile_rows = kNodeTileRows;
        q[i].n_parts = nd->n;
        q[i].part = i;
        rows[i] = mirt_params_out_rows(&q[i]);
        if (rows[i] > max_rows) max_rows = rows[i];
    }
    return max_rows;
}

// The tail of a frame on `tail` (a stream of member 0's device): members fill their parts, the parts reach member 0, the assembly
// writes `d_out`.  Params are checked by the caller (mirt_node_render / _accum_frame / _device) except what the member contexts check
// themselves.
int node_frame(MirtNode* nd, const MirtParams* p, uint32_t* d_out, hipStream_t tail, Fill fill)
{
    const uint32_t n = nd->n;
    const uint32_t w = p->width;
    MirtParams q[MIRT_NODE_MAX_MEMBERS];
    uint32_t rows[MIRT_NODE_MAX_MEMBERS];
    const uint32_t max_rows = member_params(nd, p, q, rows);
    const bool rccl = nd->transport == 1;
    const size_t slot_px = (size_t)max_rows * w;

    // buffers (grow-only).  Growing frees a buffer an earlier frame's assembly may still read: wait for that assembly first.
    bool must_grow = rccl && n * slot_px > nd->cap_gather;
    for (uint32_t i = 0; i < n; ++i)
        if ((rccl || rows[i]) && (rccl ? slot_px : (size_t)rows[i] * w) > nd->cap_part[i]) must_grow = true;
    if (must_grow && nd->consumed_pending) {
        NODE_HIP_TRY(hipSetDevice(nd->device[0]));
        NODE_HIP_TRY(hipEventSynchronize(nd->ev_consumed));
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (!rccl && !rows[i]) continue;
        NODE_HIP_TRY(hipSetDevice(nd->device[i]));
        const int rc = grow(&nd->d_part[i], &nd->cap_part[i], rccl ? slot_px : (size_t)rows[i] * w);
        if (rc != MIRT_OK) return rc;
    }
    if (rccl) {
        NODE_HIP_TRY(hipSetDevice(nd->device[0]));
        const int rc = grow(&nd->d_gather, &nd->cap_gather, n * slot_px);
        if (rc != MIRT_OK) return rc;
    }

    // members: part i on member i's stream, after the previous frame's assembly has read the part buffers
    for (uint32_t i = 0; i < n; ++i) {
        if (!rows[i] && !rccl) continue;                          // no rows: skipped (RCCL: it still takes part in the gather)
        NODE_HIP_TRY(hipSetDevice(nd->device[i]));
        if (nd->consumed_pending) NODE_HIP_TRY(hipStreamWaitEvent(nd->stream[i], nd->ev_consumed, 0));
        if (rows[i]) {
            const int rc = fill_part(fill, nd->ctx[i], &q[i], nd->d_part[i], (size_t)rows[i] * w * 4, nd->stream[i]);
            if (rc != MIRT_OK) return rc;
        }
        NODE_HIP_TRY(hipEventRecord(nd->ev_done[i], nd->stream[i]));
    }

    mirt::AssembleArgs a{};
    if (rccl) {
        // all parts ready on member 0's stream -> the gather -> the tail
        NODE_HIP_TRY(hipSetDevice(nd->device[0]));
        for (uint32_t i = 1; i < n; ++i) NODE_HIP_TRY(hipStreamWaitEvent(nd->stream[0], nd->ev_done[i], 0));
        NODE_HIP_TRY(hipEventRecord(nd->ev_gather_begin, nd->stream[0]));
        const Rccl& r = *nd->rccl;
        ncclResult_t nr = r.group_start();
        for (uint32_t i = 0; i < n && nr == ncclSuccess; ++i)
            nr = r.gather(nd->d_part[i], i == 0 ? nd->d_gather : nullptr, slot_px * 4, ncclUint8, 0, nd->comm[i], nd->stream[i]);
        const ncclResult_t ne = r.group_end();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess) return mirt::set_error(MIRT_ERR_HIP, "RCCL: %s", r.error_string(nr));
        NODE_HIP_TRY(hipSetDevice(nd->device[0]));
        NODE_HIP_TRY(hipEventRecord(nd->ev_gather_end, nd->stream[0]));
        nd->gather_timed = true;
        NODE_HIP_TRY(hipStreamWaitEvent(tail, nd->ev_gather_end, 0));
        for (uint32_t i = 0; i < n; ++i) a.parts[i] = nd->d_gather + i * slot_px;
    } else {
        NODE_HIP_TRY(hipSetDevice(nd->device[0]));
        for (uint32_t i = 0; i < n; ++i) {
            if (!rows[i]) continue;
            NODE_HIP_TRY(hipStreamWaitEvent(tail, nd->ev_done[i], 0));
            a.parts[i] = nd->d_part[i];
        }
        nd->gather_timed = false;
    }

    // assembly on the tail stream; its end releases the part buffers for the next frame
    const uint32_t rb = p->row_begin, re = p->row_end == 0 ? p->height : p->row_end;
    a.out = d_out;
    a.part_stride_px = 0;                                          // table form
    a.width = w;
    a.band_rows = re - rb;
    a.tile_rows = kNodeTileRows;
    a.n_parts = n;
    bool aligned = w % 4 == 0 && (uintptr_t)d_out % 16 == 0;
    for (uint32_t i = 0; i < n; ++i) aligned = aligned && (uintptr_t)a.parts[i] % 16 == 0;
    a.vec4 = aligned ? 1u : 0u;
    NODE_HIP_TRY(mirt::exact_build::launch_assemble(a, mirt::LaunchOn(tail, nd->ev_asm_begin, nd->ev_asm_end)));
    nd->asm_timed = true;
    NODE_HIP_TRY(hipEventRecord(nd->ev_consumed, tail));
    nd->consumed_pending = true;
    return MIRT_OK;
}

// What both render calls check before anything is queued.
int check_node_params(const MirtNode* nd, const MirtParams* p, const void* out, size_t out_len, size_t* need)
{
    if (!nd || !p || !out) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/params/output is null");
    if (!nd->have_scene) return mirt::set_error(MIRT_ERR_NO_SCENE, "mirt_node_set_scene has not succeeded");
    if (p->tile_rows != 0 || p->n_parts != 0 || p->part != 0)
        return mirt::set_error(MIRT_ERR_BAD_ROWS, "the node owns the partition: tile_rows, n_parts and part must be 0 (got %u, %u, %u)",
                               p->tile_rows, p->n_parts, p->part);
    if (p->width == 0 || p->height == 0)
        return mirt::set_error(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", p->width, p->height);
    const uint32_t rows = mirt_params_out_rows(p);
    if (rows == 0) return mirt::set_error(MIRT_ERR_BAD_ROWS, "invalid row selection [%u,%u) of %u", p->row_begin, p->row_end, p->height);
    *need = (size_t)rows * p->width * 4;
    if (out_len < *need) return mirt::set_error(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %zu needed", out_len, *need);
    return MIRT_OK;
}

}  // namespace

extern "C" {

int mirt_node_create(const int* devices, uint32_t n, uint32_t flags, MirtNode** out)
{
    if (!devices || !out) return mirt::set_error(MIRT_ERR_NULL_POINTER, "devices/out is null");
    *out = nullptr;
    // the list's shape first: no HIP call before it is known to be usable
    if (n == 0) return mirt::set_error(MIRT_ERR_NO_DEVICE, "empty device list");
    if (n > MIRT_NODE_MAX_MEMBERS)
        return mirt::set_error(MIRT_ERR_NO_DEVICE, "%u devices: a node has at most %d members", n, MIRT_NODE_MAX_MEMBERS);
    bool all_same = true, all_distinct = true;
    for (uint32_t i = 0; i < n; ++i) {
        if (devices[i] < 0) return mirt::set_error(MIRT_ERR_NO_DEVICE, "device %d is not a device ordinal", devices[i]);
        if (devices[i] != devices[0]) all_same = false;
        for (uint32_t j = 0; j < i; ++j)
            if (devices[j] == devices[i]) all_distinct = false;
    }
    if (!all_same && !all_distinct)
        return mirt::set_error(MIRT_ERR_NO_DEVICE, "mixed device list: the entries must all name one device (loopback) or all differ (RCCL)");
    if ((flags & MIRT_NODE_RCCL) && !all_distinct)
        return mirt::set_error(MIRT_ERR_NO_DEVICE, "MIRT_NODE_RCCL on a repeated device: RCCL refuses two ranks on one device");
    const bool rccl = all_distinct && (n > 1 || (flags & MIRT_NODE_RCCL));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return mirt::set_error(MIRT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    for (uint32_t i = 0; i < n; ++i)
        if (devices[i] >= count) return mirt::set_error(MIRT_ERR_NO_DEVICE, "device %d out of range (0..%d)", devices[i], count - 1);
    const Rccl* r = nullptr;
    if (rccl && !(r = load_rccl())) return MIRT_ERR_HIP;           // (load_rccl has set the message)

    MirtNode* nd = new (std::nothrow) MirtNode();
    if (!nd) return mirt::set_error(MIRT_ERR_ALLOC, "out of host memory");
    nd->n = n;
    nd->transport = rccl ? 1u : 0u;
    nd->rccl = r;
    int rc = MIRT_OK;
    for (uint32_t i = 0; i < n && rc == MIRT_OK; ++i) {
        nd->device[i] = devices[i];
        rc = mirt_ctx_create(devices[i], &nd->ctx[i]);
        void* s = nullptr;
        if (rc == MIRT_OK) rc = mirt_ctx_frame_stream(nd->ctx[i], 0, &s);
        nd->stream[i] = (hipStream_t)s;
        if (rc == MIRT_OK && (hipSetDevice(devices[i]) != hipSuccess || hipEventCreateWithFlags(&nd->ev_done[i], hipEventDisableTiming) != hipSuccess))
            rc = mirt::set_error(MIRT_ERR_HIP, "event creation on device %d failed", devices[i]);
    }
    if (rc == MIRT_OK) {
        hipError_t e = hipSetDevice(devices[0]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&nd->root_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&nd->ev_consumed, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreate(&nd->ev_asm_begin);
        if (e == hipSuccess) e = hipEventCreate(&nd->ev_asm_end);
        if (e == hipSuccess) e = hipEventCreate(&nd->ev_gather_begin);
        if (e == hipSuccess) e = hipEventCreate(&nd->ev_gather_end);
        if (e != hipSuccess) rc = mirt::set_error(MIRT_ERR_HIP, "node creation failed: %s", hipGetErrorString(e));
    }
    if (rc == MIRT_OK && rccl) {
        const ncclResult_t nr = r->comm_init_all(nd->comm, (int)n, nd->device);
        if (nr != ncclSuccess) {
            for (uint32_t i = 0; i < n; ++i) nd->comm[i] = nullptr;
            rc = mirt::set_error(MIRT_ERR_HIP, "RCCL: %s", r->error_string(nr));
        }
    }
    if (rc != MIRT_OK) {
        mirt_node_destroy(nd);
        return rc;
    }
    (void)hipSetDevice(devices[0]);
    *out = nd;
    return MIRT_OK;
}

void mirt_node_destroy(MirtNode* nd)
{
    if (!nd) return;
    // everything queued: the members' renders and gathers, the last assembly (which may sit on a caller's stream)
    for (uint32_t i = 0; i < nd->n; ++i)
        if (nd->stream[i]) { (void)hipSetDevice(nd->device[i]); (void)hipStreamSynchronize(nd->stream[i]); }
    (void)hipSetDevice(nd->device[0]);
    if (nd->consumed_pending) (void)hipEventSynchronize(nd->ev_consumed);
    if (nd->root_stream) (void)hipStreamSynchronize(nd->root_stream);
    for (uint32_t i = 0; i < nd->n; ++i)
        if (nd->comm[i]) (void)nd->rccl->comm_destroy(nd->comm[i]);
    for (uint32_t i = 0; i < nd->n; ++i) {
        (void)hipSetDevice(nd->device[i]);
        (void)hipFree(nd->d_part[i]);
        if (nd->ev_done[i]) (void)hipEventDestroy(nd->ev_done[i]);
    }
    (void)hipSetDevice(nd->device[0]);
    (void)hipFree(nd->d_gather);
    (void)hipFree(nd->d_out);
    for (hipEvent_t ev : { nd->ev_consumed, nd->ev_asm_begin, nd->ev_asm_end, nd->ev_gather_begin, nd->ev_gather_end })
        if (ev) (void)hipEventDestroy(ev);
    if (nd->root_stream) (void)hipStreamDestroy(nd->root_stream);
    for (uint32_t i = 0; i < nd->n; ++i) mirt_ctx_destroy(nd->ctx[i]);
    delete nd;
}

int mirt_node_set_scene(MirtNode* nd, const MirtScene* scene)
{
    if (!nd || !scene) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/scene is null");
    nd->have_scene = false;
    for (uint32_t i = 0; i < nd->n; ++i) {
        const int rc = mirt_ctx_set_scene(nd->ctx[i], scene);
        if (rc != MIRT_OK) return rc;
    }
    nd->have_scene = true;
    return MIRT_OK;
}

int mirt_node_set_scene_ex(MirtNode* nd, const MirtScene* scene, uint32_t flags)
{
    if (!nd || !scene) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/scene is null");
    if ((flags & ~(uint32_t)(MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE)) || flags == MIRT_SCENE_BVH_DEVICE)     // the device builder only with MIRT_SCENE_HBM
        return mirt::set_error(MIRT_ERR_BAD_MODE, "unknown set_scene_ex flags 0x%x", flags);
    nd->have_scene = false;
    for (uint32_t i = 0; i < nd->n; ++i) {
        const int rc = mirt_ctx_set_scene_ex(nd->ctx[i], scene, flags);
        if (rc != MIRT_OK) return rc;
    }
    nd->have_scene = true;
    return MIRT_OK;
}

int mirt_node_update_spheres(MirtNode* nd, uint32_t first, uint32_t count, const MirtSphere* spheres)
{
    if (!nd) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node is null");
    if (count && !spheres) return mirt::set_error(MIRT_ERR_NULL_POINTER, "spheres is null");
    if (!nd->have_scene) return mirt::set_error(MIRT_ERR_NO_SCENE, "mirt_node_set_scene has not succeeded");
    for (uint32_t i = 0; i < nd->n; ++i) {
        const int rc = mirt_ctx_update_spheres(nd->ctx[i], first, count, spheres);
        if (rc == MIRT_OK) continue;
        // every member holds the same scene, so an argument error comes from the first member and has changed nothing; any other
        // failure leaves members that disagree
        if (i > 0 || rc == MIRT_ERR_HIP || rc == MIRT_ERR_ALLOC) nd->have_scene = false;
        return rc;
    }
    return MIRT_OK;
}

int mirt_node_set_spheres(MirtNode* nd, const MirtSphere* spheres, uint32_t n_spheres)
{
    if (!nd) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node is null");
    if (n_spheres && !spheres) return mirt::set_error(MIRT_ERR_NULL_POINTER, "spheres is null");
    if (!nd->have_scene) return mirt::set_error(MIRT_ERR_NO_SCENE, "mirt_node_set_scene has not succeeded");
    for (uint32_t i = 0; i < nd->n; ++i) {
        const int rc = mirt_ctx_set_spheres(nd->ctx[i], spheres, n_spheres);
        if (rc == MIRT_OK) continue;
        // as in mirt_node_update_spheres: an argument error comes from the first member and has changed nothing
        if (i > 0 || rc == MIRT_ERR_HIP || rc == MIRT_ERR_ALLOC) nd->have_scene = false;
        return rc;
    }
    return MIRT_OK;
}

int mirt_node_set_camera(MirtNode* nd, const MirtGpuCamera* camera)
{
    if (!nd || !camera) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/camera is null");
    if (!nd->have_scene) return mirt::set_error(MIRT_ERR_NO_SCENE, "mirt_node_set_scene has not succeeded");
    for (uint32_t i = 0; i < nd->n; ++i) {
        const int rc = mirt_ctx_set_camera(nd->ctx[i], camera);
        if (rc != MIRT_OK) return rc;
    }
    return MIRT_OK;
}

static int refuse_legacy_stream(const void* hip_stream)
{
    if ((hipStream_t)hip_stream == hipStreamLegacy)
        return mirt::set_error(MIRT_ERR_HIP, "the node does not order work on hipStreamLegacy: pass a stream of your own, or NULL");
    return MIRT_OK;
}

// Both device forms: the band into `d_out`, asynchronously.
static int node_frame_device(MirtNode* nd, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream, Fill fill)
{
    if (nd->n == 1 && nd->transport == 0) {                        // one member on one device: the band straight into the output
        nd->asm_timed = nd->gather_timed = false;
        return fill_part(fill, nd->ctx[0], p, d_out, out_len, hip_stream ? hip_stream : (void*)nd->root_stream);
    }
    return node_frame(nd, p, (uint32_t*)d_out, hip_stream ? (hipStream_t)hip_stream : nd->root_stream, fill);
}

// Both host forms: the band into the node's own buffer, one D2H copy, blocking.
static int node_frame_host(MirtNode* nd, const MirtParams* p, uint8_t* out, size_t need, Fill fill)
{
    int rc;
    NODE_HIP_TRY(hipSetDevice(nd->device[0]));
    if ((rc = grow(&nd->d_out, &nd->cap_out, need / 4)) != MIRT_OK) return rc;
    if ((rc = node_frame_device(nd, p, nd->d_out, need, nullptr, fill)) != MIRT_OK) return rc;
    NODE_HIP_TRY(hipSetDevice(nd->device[0]));
    NODE_HIP_TRY(hipMemcpyAsync(out, nd->d_out, need, hipMemcpyDeviceToHost, nd->root_stream));
    NODE_HIP_TRY(hipStreamSynchronize(nd->root_stream));
    return MIRT_OK;
}

int mirt_node_render_device(MirtNode* nd, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream)
{
    size_t need = 0;
    int rc = check_node_params(nd, p, d_out, out_len, &need);
    if (rc == MIRT_OK) rc = refuse_legacy_stream(hip_stream);
    if (rc != MIRT_OK) return rc;
    return node_frame_device(nd, p, d_out, out_len, hip_stream, kFillRender);
}

int mirt_node_render(MirtNode* nd, const MirtParams* p, uint8_t* out, size_t out_len)
{
    size_t need = 0;
    int rc = check_node_params(nd, p, out, out_len, &need);
    if (rc != MIRT_OK) return rc;
    if (nd->n == 1 && nd->transport == 0) {
        nd->asm_timed = nd->gather_timed = false;
        return mirt_ctx_render(nd->ctx[0], p, out, out_len);
    }
    return node_frame_host(nd, p, out, need, kFillRender);
}

// ---- progressive accumulation on a node ----

int mirt_node_accum_reset(MirtNode* nd, const MirtParams* p)
{
    if (!nd || !p) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/params is null");
    size_t need = 0;
    int rc = check_node_params(nd, p, p, SIZE_MAX, &need);         // (no output here: scene, partition, viewport and rows)
    if (rc != MIRT_OK) return rc;
    nd->accum_valid = false;
    nd->accum_samples = 0;
    MirtParams q[MIRT_NODE_MAX_MEMBERS];
    uint32_t rows[MIRT_NODE_MAX_MEMBERS];
    (void)member_params(nd, p, q, rows);
    for (uint32_t i = 0; i < nd->n; ++i) {
        if (!rows[i]) continue;                                    // a member without rows owns no sums
        if ((rc = mirt_ctx_accum_reset(nd->ctx[i], &q[i])) != MIRT_OK) return rc;
    }
    nd->accum_params = *p;
    nd->accum_valid = true;
    return MIRT_OK;
}

// What both frame calls check after check_node_params: the sums exist and have this geometry.
static int check_node_accum(const MirtNode* nd, const MirtParams* p)
{
    const MirtParams& r = nd->accum_params;
    if (!nd->accum_valid || r.width != p->width || r.height != p->height || r.row_begin != p->row_begin ||
        (r.row_end == 0 ? r.height : r.row_end) != (p->row_end == 0 ? p->height : p->row_end))
        return mirt::set_error(MIRT_ERR_OUT_BUFFER, "accumulation buffer does not match these params: call mirt_node_accum_reset first");
    return MIRT_OK;
}

// After the members' calls: the count follows the members' (they advance together), a failure invalidates the accumulation.
static int node_accum_done(MirtNode* nd, const MirtParams* p, int rc)
{
    if (rc != MIRT_OK) {
        nd->accum_valid = false;
        nd->accum_samples = 0;
        return rc;
    }
    nd->accum_samples += p->spp;
    return MIRT_OK;
}

// A refusal a member would give before it queues anything leaves the accumulation as it is: every member with rows is asked first,
// with the context's own rules (mirt::check_accum_frame), before a frame is queued on any.
static int precheck_node_frame(MirtNode* nd, const MirtParams* p)
{
    MirtParams q[MIRT_NODE_MAX_MEMBERS];
    uint32_t rows[MIRT_NODE_MAX_MEMBERS];
    (void)member_params(nd, p, q, rows);
    for (uint32_t i = 0; i < nd->n; ++i) {
        if (!rows[i]) continue;
        const int rc = mirt::check_accum_frame(nd->ctx[i], &q[i]);
        if (rc != MIRT_OK) return rc;
    }
    return MIRT_OK;
}

int mirt_node_accum_frame_device(MirtNode* nd, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream)
{
    size_t need = 0;
    int rc = check_node_params(nd, p, d_out, out_len, &need);
    if (rc == MIRT_OK) rc = check_node_accum(nd, p);
    if (rc == MIRT_OK) rc = precheck_node_frame(nd, p);
    if (rc == MIRT_OK) rc = refuse_legacy_stream(hip_stream);
    if (rc != MIRT_OK) return rc;
    return node_accum_done(nd, p, node_frame_device(nd, p, d_out, out_len, hip_stream, kFillAccumFrame));
}

int mirt_node_accum_frame(MirtNode* nd, const MirtParams* p, uint8_t* out, size_t out_len)
{
    size_t need = 0;
    int rc = check_node_params(nd, p, out, out_len, &need);
    if (rc == MIRT_OK) rc = check_node_accum(nd, p);
    if (rc == MIRT_OK) rc = precheck_node_frame(nd, p);
    if (rc != MIRT_OK) return rc;
    return node_accum_done(nd, p, node_frame_host(nd, p, out, need, kFillAccumFrame));
}

uint32_t mirt_node_accum_samples(const MirtNode* nd) { return (nd && nd->accum_valid) ? nd->accum_samples : 0u; }

int mirt_node_accum_read(MirtNode* nd, uint64_t* out_sums, size_t out_len_u64)
{
    if (!nd || !out_sums) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/out is null");
    if (!nd->accum_valid) return mirt::set_error(MIRT_ERR_NO_SCENE, "nothing accumulated yet");
    const MirtParams* p = &nd->accum_params;
    const size_t w = p->width;
    if (out_len_u64 < (size_t)mirt_params_out_rows(p) * w * 3) return mirt::set_error(MIRT_ERR_OUT_BUFFER, "output buffer too small");
    MirtParams q[MIRT_NODE_MAX_MEMBERS];
    uint32_t rows[MIRT_NODE_MAX_MEMBERS];
    const uint32_t max_rows = member_params(nd, p, q, rows);
    std::vector<uint64_t> part((size_t)max_rows * w * 3);
    for (uint32_t i = 0; i < nd->n; ++i) {
        if (!rows[i]) continue;
        const int rc = mirt_ctx_accum_read(nd->ctx[i], part.data(), part.size());
        if (rc != MIRT_OK) return rc;
        for (uint32_t r = 0; r < rows[i]; ++r) {                   // compact row r of part i -> its row of the band
            const uint32_t band_row = mirt_params_out_row_index(&q[i], r) - p->row_begin;
            std::copy(part.begin() + (size_t)r * w * 3, part.begin() + (size_t)(r + 1) * w * 3, out_sums + (size_t)band_row * w * 3);
        }
    }
    return MIRT_OK;
}

int mirt_node_context(MirtNode* nd, uint32_t i, MirtContext** out)
{
    if (!nd || !out) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/out is null");
    if (i >= nd->n) return mirt::set_error(MIRT_ERR_BAD_ROWS, "the node has members 0..%u, not %u", nd->n - 1, i);
    *out = nd->ctx[i];
    return MIRT_OK;
}

int mirt_node_get_stats(MirtNode* nd, MirtNodeStats* out)
{
    if (!nd || !out) return mirt::set_error(MIRT_ERR_NULL_POINTER, "node/out is null");
    MirtNodeStats s{};
    s.n_members = nd->n;
    s.transport = nd->transport;
    NODE_HIP_TRY(hipSetDevice(nd->device[0]));
    float ms = 0.0f;
    if (nd->asm_timed) {
        NODE_HIP_TRY(hipEventSynchronize(nd->ev_asm_end));
        NODE_HIP_TRY(hipEventElapsedTime(&ms, nd->ev_asm_begin, nd->ev_asm_end));
        s.assemble_ms = ms;
    }
    if (nd->gather_timed) {
        NODE_HIP_TRY(hipEventSynchronize(nd->ev_gather_end));
        NODE_HIP_TRY(hipEventElapsedTime(&ms, nd->ev_gather_begin, nd->ev_gather_end));
        s.gather_ms = ms;
    }
    *out = s;
    return MIRT_OK;
}

}  // extern "C"
