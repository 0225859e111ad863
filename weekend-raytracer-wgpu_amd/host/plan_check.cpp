// plan_check — prints the launch plan (csrc/mirt_launch_plan.h) of every case of a text file, one line per case.  Host arithmetic only:
// no device is initialised.  tests/test_launch_plan.py compares the output with tests/golden/launch_plans_v1.txt.
//
// A case is one line of key=value words (anything after '#' is ignored); a key that is absent keeps its default:
//   name                                   the case's label, repeated in front of its plan
//   cu ldscu ldsblk                        PlanFacts: device
//   ns nm nr img sky flat hbm              ... scene: spheres, materials, shading routines, image texture, sky, fits_flat, hbm
//   gb gpk gfy shd  dep  pin               ... grid bytes / packable / flat-y / shade records; tree depth; pinhole camera
//   w h spp nb mode fl(hex) rb re tr np part sb fspp fb     MirtParams
//   t.<field>                              a Tuning field that differs from its default (t.pool_min_spp=40)
//   frame res                              the frame bit of plan_render; resident_per_cu of plan_blocks
//
// plan_check --kernels CASES.txt prints the kernel of every case instead (tests/test_launch_kernels.py), four words per line: the case, the name
// mirt_ctx_last_kernel would report (plan_kernel_name), the template instance render_kernel selects in the plan's build -- the symbol of
// its kernel handle in libmirt.so, demangled and written as the reported names are --, and that symbol itself.  "-": no such instance.
//
// plan_check --queries CASES.txt / --query-kernels CASES.txt do the same for the query launches (QueryPlan, query_kernel; tests/test_query_plan.py).
// A case gives the facts, the tuning and res as above and
//   q                                      trace / features / radiance / adapt: the planning function (the plan chooses the pooled and LDS families)
//   n  qf(hex)                             rays; the MIRT_RAYS_* / MIRT_FEATURES_* / MIRT_RADIANCE_* bits (radiance: spp, sb, nb as MirtParams')
//   af(hex) run px                         adapt: MirtAdaptParams.flags, a step of a run, pixels in the buffer; fl = the step's MIRT_FLAG_* bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <cxxabi.h>
#include <dlfcn.h>

#include "../csrc/mirt_launch_plan.h"

// mirt_kernels.h (not included: it needs the HIP headers) declares these; a kernel's handle is all this program wants of them
namespace mirt {
struct RenderArgs;
using RenderKernel = void (*)(RenderArgs);
namespace exact_build { RenderKernel render_kernel(const RenderPlan& plan); const void* query_kernel(const QueryPlan& plan); }
namespace fast_build { RenderKernel render_kernel(const RenderPlan& plan); }
}

static const char* const kKernelNames[] = { "parity", "parity-hbm", "pt-strip", "pt-hbm", "pt-pool", "pt-pool-hbm" };

// a list with its runs folded: 0,105024,154176x4
static void print_list(FILE* out, const char* key, const uint32_t* v, uint32_t n)
{
    fprintf(out, " %s=", key);
    for (uint32_t i = 0, run; i < n; i += run) {
        for (run = 1; i + run < n && v[i + run] == v[i]; ++run) {}
        fprintf(out, run > 1 ? "%s%ux%u" : "%s%u", i ? "," : "", v[i], run);
    }
}

// The plan in its fixed one-line format.  id = fast count hosek frame use_grid hbm_bvh by_pixel stream; cfg = pool_cfg/pool_nq; pool = threads/slots/lds;
// sch = static_units stream_samples strip_cand grid_flat_y spread_units pinhole; gps = grid_pool_slots; lt = launch_threads; bse = bvh_stack_entries;
// fd / dt = first_dispensed / disp_taken.  A refused launch prints its status and message instead.
static void print_plan(FILE* out, const char* name, const mirt::RenderPlan& p)
{
    if (p.status != MIRT_OK) { fprintf(out, "%s status=%d %s\n", name, p.status, p.message); return; }
    fprintf(out, "%s %s id=%d%d%d%d%d%d%d%d cfg=%u/%u pool=%u/%u/%u rows=%u units=%u", name, kKernelNames[p.kernel], p.fast, p.count, p.hosek, p.frame,
            p.use_grid, p.hbm_bvh, p.by_pixel, p.stream, p.pool_cfg, p.pool_nq, p.pool.threads, p.pool.slots, p.pool.lds_bytes, p.out_rows, p.n_units);
    print_list(out, "lu", p.lvl_unit, mirt::kStripLevels + 1);
    print_list(out, "lp", p.lvl_pix, mirt::kStripLevels + 1);
    fprintf(out, " pxg=%u sch=%u%u%u%u%u%u gps=%u lt=%u lds=%u bse=%u blocks=%u fd=%u", p.px_groups_log2, p.static_units, p.stream_samples, p.strip_cand, p.grid_flat_y,
            p.spread_units, p.pinhole, p.grid_pool_slots, p.launch_threads, p.lds_bytes, p.bvh_stack_entries, p.blocks, p.first_dispensed);
    print_list(out, "dt", p.disp_taken, 8);
    fputc('\n', out);
}

static void erase_all(std::string& s, const char* what)
{
    for (size_t at; (at = s.find(what)) != std::string::npos;) s.erase(at, std::strlen(what));
}

// "void mirt::exact_build::render_pt_pool_kernel<256u, 112u, 6u, false, false, 3u, false, false>(mirt::RenderArgs)" as a reported name is
// written: no return type, no argument list, no "mirt::exact_build::" (the fast build keeps "fast_build::"), no spaces, no unsigned suffixes
static std::string as_reported(const char* demangled)
{
    std::string s = demangled;
    if (s.rfind("void ", 0) == 0) s.erase(0, 5);
    const size_t args = s.find('(');       // (template arguments are numbers and bools; a query kernel's argument list has parentheses of its own)
    if (args != std::string::npos) s.erase(args);
    erase_all(s, "mirt::exact_build::");
    erase_all(s, "mirt::");
    erase_all(s, "__device_stub__");
    erase_all(s, " ");
    for (size_t i = 1; i + 1 < s.size(); ++i)
        if (s[i] == 'u' && s[i - 1] >= '0' && s[i - 1] <= '9' && (s[i + 1] == ',' || s[i + 1] == '>')) s.erase(i, 1);
    return s;
}

// case, reported name, the instance behind the handle `k` written as a reported name, its symbol
static void print_handle(FILE* out, const char* name, const char* reported, const void* k)
{
    Dl_info info{};
    if (!k || !dladdr(k, &info) || !info.dli_sname || info.dli_saddr != k) {
        fprintf(out, "%s %s - -\n", name, reported);
        return;
    }
    int status = 0;
    char* const demangled = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    fprintf(out, "%s %s %s %s\n", name, reported, status == 0 ? as_reported(demangled).c_str() : "-", info.dli_sname);
    std::free(demangled);
}

static void print_kernel(FILE* out, const char* name, const mirt::RenderPlan& p)
{
    if (p.status != MIRT_OK) { fprintf(out, "%s status=%d %s\n", name, p.status, p.message); return; }
    char reported[128];
    mirt::plan_kernel_name(p, reported, sizeof reported);
    print_handle(out, name, reported, reinterpret_cast<const void*>(p.fast ? mirt::fast_build::render_kernel(p) : mirt::exact_build::render_kernel(p)));
}

static void print_query_kernel(FILE* out, const char* name, const mirt::QueryPlan& p)
{
    if (p.status != MIRT_OK) { fprintf(out, "%s status=%d %s\n", name, p.status, p.message); return; }
    char reported[128];
    mirt::query_kernel_name(p, reported, sizeof reported);
    print_handle(out, name, reported, mirt::exact_build::query_kernel(p));
}

// ---- query launches (plan_check --queries / --query-kernels; tests/test_query_plan.py) ----
static const char* const kFamilyNames[] = { "trace", "features", "radiance", "radiance-pool", "adapt", "adapt-pool", "adapt-lds", "trace-lds", "features-lds", "radiance-lds" };

// The query plan in its fixed one-line format.  id = bvh any count sorted hosek grid run; geo = threads/slots/min waves; bse = bvh_stack_entries;
// pxg = px_groups_log2; row = rays_as_row; cap = cu_count/blocks_per_cu/at_most_blocks.  A refused launch prints its status and message instead.
static void print_query_plan(FILE* out, const char* name, const mirt::QueryPlan& p)
{
    if (p.status != MIRT_OK) { fprintf(out, "%s status=%d %s\n", name, p.status, p.message); return; }
    fprintf(out, "%s %s id=%d%d%d%d%d%d%d geo=%u/%u/%u lds=%u bse=%u units=%u pxg=%u row=%d n=%u blocks=%u cap=%u/%u/%u\n", name, kFamilyNames[p.family], p.bvh, p.any,
            p.count, p.sorted, p.hosek, p.grid, p.run, p.threads, p.slots, p.min_waves, p.lds_bytes, p.bvh_stack_entries, p.n_units, p.px_groups_log2, p.rays_as_row,
            p.n_rays, p.blocks, p.cu_count, p.blocks_per_cu, p.at_most_blocks);
}

struct Case {
    char             name[64] = "?";
    mirt::PlanFacts  f{};
    mirt::Tuning     t;
    MirtParams       p{};
    uint32_t         frame = 0, res = 0;
    // a query case: q = trace / features / radiance / adapt; n rays; qf = the MIRT_RAYS_* / MIRT_FEATURES_* / MIRT_RADIANCE_* bits (radiance: spp,
    // sb and nb are the params'); adapt: fl = the step's MIRT_FLAG_* bits, af = MirtAdaptParams.flags, run, px = pixels in the buffer
    char             q[16] = "";
    uint32_t         n = 0, qf = 0, af = 0, run = 0;
    uint64_t         px = 0;
};

static bool plan_query(const Case& c, mirt::QueryPlan* plan)
{
    const MirtRadianceParams rp{ c.p.spp, c.p.sample_begin, c.p.num_bounces, c.qf, c.p.seed };
    if (std::strcmp(c.q, "trace") == 0) *plan = mirt::plan_trace(c.f, c.t, c.n, c.qf);
    else if (std::strcmp(c.q, "features") == 0) *plan = mirt::plan_features(c.f, c.t, c.p, c.qf);
    else if (std::strcmp(c.q, "radiance") == 0) *plan = mirt::plan_radiance(c.f, c.t, c.n, rp);
    else if (std::strcmp(c.q, "adapt") == 0) *plan = mirt::plan_adapt(c.f, c.t, c.p, c.af, c.run != 0u, c.px);
    else return false;
    if (plan->status == MIRT_OK) mirt::query_plan_blocks(*plan, c.res);
    return true;
}

enum FieldType { kU32, kU64, kInt, kBool, kDouble, kHex };
struct Field { const char* key; FieldType type; void* at; };

static bool set_field(Case& c, const char* key, const char* val)
{
    mirt::PlanFacts& f = c.f; mirt::Tuning& t = c.t; MirtParams& p = c.p;
    const Field fields[] = {
        { "cu", kU32, &f.cu_count }, { "ldscu", kU64, &f.lds_per_cu }, { "ldsblk", kU64, &f.lds_per_block },
        { "ns", kU32, &f.n_spheres }, { "nm", kU32, &f.n_mats }, { "nr", kU32, &f.n_shading_routines }, { "img", kBool, &f.has_image_texture },
        { "sky", kBool, &f.have_sky }, { "flat", kBool, &f.fits_flat }, { "hbm", kBool, &f.hbm }, { "gb", kU32, &f.grid_bytes },
        { "gpk", kBool, &f.grid_packable }, { "gfy", kBool, &f.grid_flat_y }, { "shd", kBool, &f.have_shade }, { "dep", kU32, &f.bvh_max_depth },
        { "pin", kBool, &f.camera_is_pinhole },
        { "w", kU32, &p.width }, { "h", kU32, &p.height }, { "spp", kU32, &p.spp }, { "nb", kU32, &p.num_bounces }, { "mode", kU32, &p.mode },
        { "fl", kHex, &p.flags }, { "rb", kU32, &p.row_begin }, { "re", kU32, &p.row_end }, { "tr", kU32, &p.tile_rows }, { "np", kU32, &p.n_parts },
        { "part", kU32, &p.part }, { "sb", kU32, &p.sample_begin }, { "fspp", kU32, &p.frame_spp }, { "fb", kU32, &p.frame_begin },
        { "t.pool_config", kInt, &t.pool_config }, { "t.pool_grid", kInt, &t.pool_grid }, { "t.fixed_strips", kBool, &t.fixed_strips },
        { "t.gss_min_width", kU32, &t.gss_min_width }, { "t.gss_keep", kDouble, &t.gss_keep }, { "t.by_pixel", kInt, &t.by_pixel },
        { "t.pool_blocks_per_cu", kU32, &t.pool_blocks_per_cu }, { "t.pinhole", kInt, &t.pinhole }, { "t.spread_units", kInt, &t.spread_units },
        { "t.static_units", kInt, &t.static_units }, { "t.pool_min_spp", kInt, &t.pool_min_spp }, { "t.stream", kInt, &t.stream },
        { "t.px_groups", kInt, &t.px_groups }, { "t.strip_cand", kInt, &t.strip_cand }, { "t.static_block", kU32, &t.static_block },
        { "t.static_grid", kInt, &t.static_grid }, { "t.hbm_pool_slots", kU32, &t.hbm_pool_slots },
        { "t.radiance_pool_blocks", kU32, &t.radiance_pool_blocks }, { "t.adapt_pool_blocks", kU32, &t.adapt_pool_blocks },
        { "t.adapt_lds_blocks", kU32, &t.adapt_lds_blocks }, { "t.adapt_lds_groups", kU32, &t.adapt_lds_groups },
        { "t.query_lds_blocks", kU32, &t.query_lds_blocks },
        { "frame", kU32, &c.frame }, { "res", kU32, &c.res },
        { "n", kU32, &c.n }, { "qf", kHex, &c.qf }, { "af", kHex, &c.af }, { "run", kU32, &c.run }, { "px", kU64, &c.px },
    };
    for (const Field& fd : fields) {
        if (std::strcmp(fd.key, key) != 0) continue;
        switch (fd.type) {
        case kU32:    *(uint32_t*)fd.at = (uint32_t)std::strtoul(val, nullptr, 10); break;
        case kU64:    *(uint64_t*)fd.at = std::strtoull(val, nullptr, 10); break;
        case kInt:    *(int*)fd.at = (int)std::strtol(val, nullptr, 10); break;
        case kBool:   *(bool*)fd.at = std::strtol(val, nullptr, 10) != 0; break;
        case kDouble: *(double*)fd.at = std::strtod(val, nullptr); break;
        case kHex:    *(uint32_t*)fd.at = (uint32_t)std::strtoul(val, nullptr, 16); break;
        }
        return true;
    }
    return false;
}

int main(int argc, char** argv)
{
    const char* const mode = argc == 3 ? argv[1] : "";
    const bool query_kernels = std::strcmp(mode, "--query-kernels") == 0, queries = query_kernels || std::strcmp(mode, "--queries") == 0;
    const bool kernels = std::strcmp(mode, "--kernels") == 0;
    if (argc != 2 && !kernels && !queries) { fprintf(stderr, "usage: plan_check [--kernels | --queries | --query-kernels] CASES.txt\n"); return 2; }
    FILE* in = std::fopen(argv[argc - 1], "r");
    if (!in) { fprintf(stderr, "plan_check: cannot open %s\n", argv[argc - 1]); return 2; }
    char line[2048];
    for (int n = 1; std::fgets(line, sizeof line, in); ++n) {
        if (char* hash = std::strchr(line, '#')) *hash = '\0';
        Case c;
        bool any = false;
        for (char* word = std::strtok(line, " \t\r\n"); word; word = std::strtok(nullptr, " \t\r\n")) {
            char* eq = std::strchr(word, '=');
            if (!eq) { fprintf(stderr, "plan_check: line %d: '%s' is not key=value\n", n, word); return 2; }
            *eq = '\0';
            any = true;
            if (std::strcmp(word, "name") == 0) snprintf(c.name, sizeof c.name, "%s", eq + 1);
            else if (std::strcmp(word, "q") == 0) snprintf(c.q, sizeof c.q, "%s", eq + 1);
            else if (!set_field(c, word, eq + 1)) { fprintf(stderr, "plan_check: line %d: unknown key '%s'\n", n, word); return 2; }
        }
        if (!any) continue;
        if (queries) {
            mirt::QueryPlan plan{};
            if (!plan_query(c, &plan)) { fprintf(stderr, "plan_check: line %d: q='%s' is no query\n", n, c.q); return 2; }
            if (query_kernels) print_query_kernel(stdout, c.name, plan);
            else print_query_plan(stdout, c.name, plan);
            continue;
        }
        mirt::RenderPlan plan = mirt::plan_render(c.f, c.t, c.p, c.frame != 0u);
        if (plan.status == MIRT_OK) mirt::plan_blocks(plan, c.res);
        if (kernels) print_kernel(stdout, c.name, plan);
        else print_plan(stdout, c.name, plan);
    }
    std::fclose(in);
    return 0;
}
