// mirt_centre_ray_text.inc -- the centre ray of pixel (x, y), as TEXT: included with `x`, `y` and the camera registers `C` in scope by
// mirt_feature_item_text.inc (whose pixel traces it) and by reproject_kernel (which carries its hit to the previous frame).
// mirt_camera_pixel_ray restates it on the host.
    const float u = ((float)x + 0.5f) * C.inv_w;
    const float v = 1.0f - ((float)y + 0.5f) * C.inv_h;
    f3 ro = C.eye;
    f3 rd = fma3(v, C.ver, fma3(u, C.hor, C.llc)) - C.eye;
