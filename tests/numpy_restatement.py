"""Independent numpy restatement of the SVGF kernels and the RNG (TEST INFRASTRUCTURE), written from the GLSL
(/root/reference/data/shaders/hybrid_render_path/svgf.comp, svgf_atrous_filter.comp, ../common.glsl) without
looking at oracle/vhr_oracle.c's structure: a second pin for the oracle (SURVEY.md section 8c 'Fixtures policy').
Vectorised over the image, so the operation order per pixel is the shader's but taps are processed image-wide."""
import numpy as np

F = np.float32


def h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def f2h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def seed_thread(seed):
    m = 0xffffffff
    seed &= m
    seed = ((seed ^ 61) ^ (seed >> 16)) & m
    seed = (seed * 9) & m
    seed = (seed ^ (seed >> 4)) & m
    seed = (seed * 0x27d4eb2d) & m
    seed = (seed ^ (seed >> 15)) & m
    return seed


def xorshift(state):
    m = 0xffffffff
    state ^= (state << 13) & m
    state ^= state >> 17
    state ^= (state << 5) & m
    return state & m


def random01(state):
    state = xorshift(state)
    bits = np.array([0x3f800000 | (state >> 9)], np.uint32)
    return state, np.float32(bits.view(np.float32)[0] - F(1.0))


def _shift(img, dx, dy, fill=0):
    """out[y, x] = img[y + dy, x + dx] where in range, else `fill`; also returns the in-range mask."""
    H, W = img.shape[:2]
    out = np.full_like(img, fill)
    ys = slice(max(0, -dy), min(H, H - dy))
    xs = slice(max(0, -dx), min(W, W - dx))
    yd = slice(max(0, -dy) + dy, min(H, H - dy) + dy)
    xd = slice(max(0, -dx) + dx, min(W, W - dx) + dx)
    mask = np.zeros((H, W), bool)
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = img[yd, xd]
        mask[ys, xs] = True
    return out, mask


def atrous(normals_bits, in_bits, step):
    n = h2f(normals_bits)
    p = h2f(in_bits)
    H, W = p.shape[:2]
    normal_p, id_p = n[..., :3], n[..., 3].astype(np.int32)
    var = np.zeros((H, W, 2), F)
    gw = [F(1 / 16), F(1 / 8), F(1 / 16), F(1 / 8), F(1 / 4), F(1 / 8), F(1 / 16), F(1 / 8), F(1 / 16)]
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            q, m = _shift(p, x, y)
            w = gw[3 * (y + 1) + (x + 1)]
            var = var + np.where(m[..., None], w * q[..., 2:4], F(0)).astype(F)
    k1 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
    sum_w = np.ones((H, W, 2), F)
    acc = p.copy()
    denom = (F(4.0) * np.sqrt(var) + F(1e-6)).astype(F)
    for y in range(-2, 3):
        for x in range(-2, 3):
            if x == 0 and y == 0:
                continue
            q, m = _shift(p, x * step, y * step)
            nq, _ = _shift(n, x * step, y * step)
            kernel = F(k1[y + 2] * k1[x + 2])
            d = ((normal_p[..., 0] * nq[..., 0] + normal_p[..., 1] * nq[..., 1]) + normal_p[..., 2] * nq[..., 2]).astype(F)
            with np.errstate(over="ignore", under="ignore"):
                pw = np.where(d > 0, d, F(0)).astype(F)
                for _ in range(7):
                    pw = (pw * pw).astype(F)
            wid = (id_p == nq[..., 3].astype(np.int32)).astype(F)
            w = ((kernel * pw) * wid).astype(F)
            e = (np.abs(p[..., 0:2] - q[..., 0:2]) / denom).astype(F)
            lw = np.exp(-e).astype(F)
            wxy = (w[..., None] * lw).astype(F)
            wxy = np.where(m[..., None], wxy, F(0)).astype(F)
            sum_w = (sum_w + wxy).astype(F)
            acc[..., 0:2] = (acc[..., 0:2] + wxy * q[..., 0:2]).astype(F)
            acc[..., 2:4] = (acc[..., 2:4] + (wxy * wxy) * q[..., 2:4]).astype(F)
    out = np.empty_like(acc)
    out[..., 0:2] = acc[..., 0:2] / sum_w
    out[..., 2:4] = acc[..., 2:4] / (sum_w * sum_w)
    return f2h(out)


def atrous_f64(normals_bits, in_bits, step, display_size=None):
    """svgf_atrous_filter.comp:17-101 in binary64: a truth of higher precision than the fp32 evaluations (the oracle, `atrous` above, the
    HIP kernels), which all share one operation order.  A true pow(max(d, 0), 128) with pow of a non-positive base = 0 (oracle decision
    v), np.exp, true divisions, ids as int(w) with a NaN id = 0 (decision viii), the shader's bounds test ((float)sx >= display_size
    skips the tap; default: the image extent), ONE rounding at the end, binary64 -> fp16 directly.

    Returns (out_bits (H, W, 4) uint16, live (H, W, 2) int): per pixel and channel (shadow, AO), the number of in-image taps whose
    binary64 weight is non-zero."""
    n = np.asarray(normals_bits, np.uint16).view(np.float16).astype(np.float64)
    p = np.asarray(in_bits, np.uint16).view(np.float16).astype(np.float64)
    H, W = p.shape[:2]
    dw, dh = (float(W), float(H)) if display_size is None else (float(display_size[0]), float(display_size[1]))
    assert dw <= W and dh <= H, "taps inside display_size must lie in the image"
    ys, xs = np.mgrid[0:H, 0:W]

    def inside(dx, dy):          # :28-29, :75-76: an int coordinate against the float display size
        sx, sy = xs + dx, ys + dy
        return (sx >= 0) & ~(sx.astype(np.float32) >= np.float32(dw)) & (sy >= 0) & ~(sy.astype(np.float32) >= np.float32(dh))

    with np.errstate(invalid="ignore"):
        ids = np.where(np.isnan(n[..., 3]), 0.0, np.trunc(n[..., 3])).astype(np.int64)
    var = np.zeros((H, W, 2))
    for y in (-1, 0, 1):                                                                   # :17-38
        for x in (-1, 0, 1):
            q, _ = _shift(p, x, y)
            g = (0.5 if x == 0 else 0.25) * (0.5 if y == 0 else 0.25)
            var = var + np.where(inside(x, y)[..., None], g * q[..., 2:4], 0.0)
    with np.errstate(invalid="ignore"):
        denom = 4.0 * np.sqrt(var) + 1e-6                                                  # :49
    k1 = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    sum_w = np.ones((H, W, 2))
    acc = p.copy()
    live = np.zeros((H, W, 2), np.int64)
    for y in range(-2, 3):
        for x in range(-2, 3):                                                             # :72-94
            if x == 0 and y == 0:
                continue
            m = inside(x * step, y * step)
            if not m.any():
                continue
            q, _ = _shift(p, x * step, y * step)
            nq, _ = _shift(n, x * step, y * step)
            idq, _ = _shift(ids, x * step, y * step)
            d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                wn = np.where(d > 0, np.power(np.where(d > 0, d, 0.0), 128.0), 0.0)       # :45 (decision v)
                w = (k1[y + 2] * k1[x + 2]) * wn * (ids == idq)                            # :89
                lw = np.exp(-(np.abs(p[..., 0:2] - q[..., 0:2]) / denom))                  # :48-50
                wxy = np.where(m[..., None], w[..., None] * lw, 0.0)
                live += wxy != 0
                sum_w = sum_w + wxy
                acc[..., 0:2] += wxy * q[..., 0:2]                                         # :94
                acc[..., 2:4] += (wxy * wxy) * q[..., 2:4]
    out = np.empty_like(acc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out[..., 0:2] = acc[..., 0:2] / sum_w
        out[..., 2:4] = acc[..., 2:4] / (sum_w * sum_w)
        return out.astype(np.float16).view(np.uint16), live


def temporal(W, H, normals_bits, motion_bits, rt_bits, prev_normals_bits, history_bits, moments_bits):
    n = h2f(normals_bits)
    mv = h2f(motion_bits)
    rt = h2f(rt_bits)
    pn = h2f(prev_normals_bits)
    hist = h2f(history_bits)
    mom = h2f(moments_bits)
    ys, xs = np.mgrid[0:H, 0:W]
    cur_n, cur_id = n[..., :3], n[..., 3].astype(np.int32)
    pcx = ((xs.astype(F) - mv[..., 0] * F(W)) + F(0.5)).astype(F)
    pcy = ((ys.astype(F) - mv[..., 1] * F(H)) + F(0.5)).astype(F)
    fx = (pcx - np.floor(pcx)).astype(F)
    fy = (pcy - np.floor(pcy)).astype(F)
    with np.errstate(invalid="ignore"):
        ax = np.where(np.isnan(pcx), 0, np.trunc(pcx)).astype(np.int64)
        ay = np.where(np.isnan(pcy), 0, np.trunc(pcy)).astype(np.int64)
    weights = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]

    def gather(sx, sy):
        inb = (sx >= 0) & (sy >= 0) & (sx < W) & (sy < H)
        cx, cy = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
        p = pn[cy, cx]
        ok = inb & (cur_id == p[..., 3].astype(np.int32))
        d = ((cur_n[..., 0] * p[..., 0] + cur_n[..., 1] * p[..., 1]) + cur_n[..., 2] * p[..., 2]).astype(F)
        ok &= ~(d < F(0.70710678118654752440084))
        return ok, hist[cy, cx], mom[cy, cx]

    z = np.zeros((H, W), F)
    ps, pa, s = z.copy(), z.copy(), z.copy()
    m0, m1, a0, a1 = z.copy(), z.copy(), z.copy(), z.copy()
    for i, (ox, oy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        ok, h, m = gather(ax + ox, ay + oy)
        w = weights[i].astype(F)
        ps = np.where(ok, ps + w * h[..., 0], ps).astype(F)
        pa = np.where(ok, pa + w * h[..., 1], pa).astype(F)
        m0 = np.where(ok, m0 + w * m[..., 0], m0).astype(F)
        m1 = np.where(ok, m1 + w * m[..., 1], m1).astype(F)
        a0 = np.where(ok, a0 + w * F(0), a0).astype(F)
        a1 = np.where(ok, a1 + w * F(1), a1).astype(F)
        s = np.where(ok, s + w, s).astype(F)
    with np.errstate(invalid="ignore"):
        valid = s > F(1e-6)
    retry = ~valid
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            ok, h, m = gather(ax + ox, ay + oy)
            ok &= retry
            ps = np.where(ok, ps + h[..., 0], ps).astype(F)
            pa = np.where(ok, pa + h[..., 1], pa).astype(F)
            m0 = np.where(ok, m0 + m[..., 0], m0).astype(F)
            m1 = np.where(ok, m1 + m[..., 1], m1).astype(F)
            a0 = np.where(ok, a0 + F(0), a0).astype(F)
            a1 = np.where(ok, a1 + F(1), a1).astype(F)
            s = np.where(ok, s + F(1), s).astype(F)
    with np.errstate(invalid="ignore"):
        valid = np.where(retry, s > F(1e-6), valid)
    cs, ca = rt[..., 0], rt[..., 1]
    sm0, sm1, am0, am1 = cs, (cs * cs).astype(F), ca, (ca * ca).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        mix = lambda a, b, t: (a * (F(1) - F(t)) + b * F(t)).astype(F)   # noqa: E731
        v_sm0, v_sm1 = mix(m0 / s, sm0, 0.2), mix(m1 / s, sm1, 0.2)
        v_am0, v_am1 = mix(a0 / s, am0, 0.2), mix(a1 / s, am1, 0.2)
        v_s, v_a = mix(ps / s, cs, 0.2), mix(pa / s, ca, 0.2)
    sm0 = np.where(valid, v_sm0, sm0)
    sm1 = np.where(valid, v_sm1, sm1)
    am0 = np.where(valid, v_am0, am0)
    am1 = np.where(valid, v_am1, am1)
    out_s = np.where(valid, v_s, cs)
    out_a = np.where(valid, v_a, ca)
    sv = np.maximum(F(0), sm1 - sm0 * sm0).astype(F)
    av = np.maximum(F(0), am1 - am0 * am0).astype(F)
    return f2h(np.stack([out_s, out_a, sv, av], -1)), f2h(np.stack([sm0, sm1], -1))


# ---------------------------------------------------------------------------------------------------------
# K2 in float64, written from the GLSL (raygen.rgen:59-65, reflection_hit.rchit:10-72, common.glsl:116-150) for untextured
# materials: a second derivation of the shading formulas, compared with the oracle at fp16 resolution.
# ---------------------------------------------------------------------------------------------------------
def _mat(pfd, name):
    return np.asarray(pfd[name], np.float64).reshape(4, 4).T          # column-major 16 floats -> math matrix


def world_position(pfd, depth, u, v):                                  # glsl_common.h:118-122
    r = _mat(pfd, "camera_viewproj_inverse") @ np.array([u * 2.0 - 1.0, v * 2.0 - 1.0, depth, 1.0])
    return r[:3] / r[3]


def reflection_ray(pfd, depth, normal, x, y, W, H, bias=0.1):           # raygen.rgen:15-16,26-29,60-63
    P = world_position(pfd, float(depth), (x + 0.5) / W, (y + 0.5) / H)
    N = np.asarray(normal, np.float64)
    cam = _mat(pfd, "camera_view_inverse")[:3, 3]
    I = (P - cam) / np.linalg.norm(P - cam)
    return P + bias * N, I - 2.0 * np.dot(N, I) * N


def interpolate_hit(scene, prim_index, tri, u, v):                      # reflection_hit.rchit:11-24
    pr = scene.primitives[prim_index]
    idx = scene.indices[int(pr["index_offset"]) + 3 * tri:int(pr["index_offset"]) + 3 * tri + 3]
    vs = scene.vertices[int(pr["vertex_offset"]) + idx]
    b = np.array([1.0 - u - v, u, v])
    normal = (np.asarray(vs["normal"], np.float64) * b[:, None]).sum(0)           # object space, unnormalised (:23)
    opos = (np.asarray(vs["pos"], np.float64) * b[:, None]).sum(0)
    M = np.asarray(pr["transform"], np.float64).reshape(4, 4).T
    return pr, normal, (M @ np.append(opos, 1.0))[:3]


def brdf_terms(albedo, metallic, roughness, N, V, L):                   # common.glsl:116-150
    H = (L + V) / np.linalg.norm(L + V)
    f0 = 0.04 * (1.0 - metallic) + albedo * metallic                    # mix(vec3(0.04), albedo, metallic)
    hv = max(np.dot(H, V), 0.0)
    F = f0 + (1.0 - f0) * (1.0 - hv) ** 5
    a2 = roughness * roughness
    nh = max(np.dot(N, H), 0.0)
    f = nh * nh * (a2 - 1.0) + 1.0
    D = a2 / (np.pi * f * f)
    k = (roughness + 1.0) ** 2 * 0.125
    nv, nl = max(np.dot(N, V), 0.0), max(np.dot(N, L), 0.0)
    G = (nv / (nv * (1.0 - k) + k)) * (nl / (nl * (1.0 - k) + k))
    specular = D * G * F / max(4.0 * nv * nl, 1e-6)
    diffuse = (1.0 - F) * (1.0 - metallic) * albedo / np.pi
    return diffuse, specular, nl


def reflection_hit(scene, pfd, prim_index, tri, u, v):                  # reflection_hit.rchit:26-71, untextured materials
    pr, N, position = interpolate_hit(scene, prim_index, tri, u, v)
    m = pr["material"]
    assert int(m["base_color_texture"]) == -1 and int(m["metallic_roughness_texture"]) == -1
    albedo = np.asarray(m["base_color"], np.float64)[:3]
    roughness = min(max(float(m["roughness_factor"]), 0.04), 1.0)
    metallic = min(max(float(m["metallic_factor"]), 0.0), 1.0)
    cam = _mat(pfd, "camera_view_inverse")[:3, 3]
    V = (cam - position) / np.linalg.norm(cam - position)
    light = pfd["directional_light"]
    L = -np.asarray(light["direction"], np.float64)[:3]
    diffuse, specular, nl = brdf_terms(albedo, metallic, roughness, N, V, L)
    return albedo * (0.2 / np.pi) + (diffuse + specular) * nl * np.asarray(light["intensity"], np.float64)[:3] * np.asarray(light["color"], np.float64)[:3]


# ---------------------------------------------------------------------------------------------------------
# Screen-space alternatives in float64, vectorised over the image, written from the GLSL (ssao.comp:14-53,
# ssao_blur.comp:11-26, ssr.comp:16-137, glsl_common.h:111-122, common.glsl:116-150): a second derivation compared with
# the oracle at a tolerance (float64 here, fp32 there; np.sin / np.cos instead of the shared polynomial).
# ---------------------------------------------------------------------------------------------------------
def seed_thread_v(seed):
    seed = np.asarray(seed, np.uint64) & 0xffffffff
    seed = ((seed ^ 61) ^ (seed >> 16)) & 0xffffffff
    seed = (seed * 9) & 0xffffffff
    seed = (seed ^ (seed >> 4)) & 0xffffffff
    seed = (seed * 0x27d4eb2d) & 0xffffffff
    seed = (seed ^ (seed >> 15)) & 0xffffffff
    return seed


def random01_v(state):
    state = state ^ ((state << 13) & 0xffffffff)
    state = state ^ (state >> 17)
    state = state ^ ((state << 5) & 0xffffffff)
    state &= 0xffffffff
    bits = (0x3f800000 | (state >> 9)).astype(np.uint32)
    return state, bits.view(np.float32).astype(np.float64) - 1.0


def sample_linear_repeat(img, u, v):
    """texture() with the default sampler (LINEAR, REPEAT, resource_manager.cpp:58-69) on an (H, W[, C]) float array."""
    H, W = img.shape[:2]
    with np.errstate(invalid="ignore"):
        fx, fy = u * W - 0.5, v * H - 0.5
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        bad = ~(np.isfinite(x0f) & np.isfinite(y0f))
        x0 = np.mod(np.where(bad, 0, np.clip(x0f, -2**31, 2**31 - 1)).astype(np.int64), W)
        y0 = np.mod(np.where(bad, 0, np.clip(y0f, -2**31, 2**31 - 1)).astype(np.int64), H)
    x1, y1 = (x0 + 1) % W, (y0 + 1) % H
    if img.ndim == 3:
        ax, ay = ax[..., None], ay[..., None]
    return (img[y0, x0] * (1 - ax) + img[y0, x1] * ax) * (1 - ay) + (img[y1, x0] * (1 - ax) + img[y1, x1] * ax) * ay


def _unproject(M, depth, u, v):
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.stack([u * 2.0 - 1.0, v * 2.0 - 1.0, depth, np.ones_like(depth)], -1) @ M.T
        return p[..., :3] / p[..., 3:4]


def _fmax(a, b):          # IEEE maxNum: a NaN operand loses (oracle decision xii)
    return np.fmax(a, b)


def _ssao_centre(pfd, depth, radius):
    """ssao.comp:15-29 of every pixel: (cu, cv, centre depth, P, the uv radius)."""
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W]
    inv = np.asarray(pfd["display_size_inverse"], np.float64)
    cu, cv = xs * inv[0], ys * inv[1]                                   # :15, uv = pixel * display_size_inverse
    cur = sample_linear_repeat(depth, cu, cv)
    Pinv = _mat(pfd, "camera_proj_inverse")
    P = _unproject(Pinv, cur, cu, cv)
    with np.errstate(divide="ignore", invalid="ignore"):
        pr = radius / P[..., 2]
    return cu, cv, cur, P, pr


def _ssao_samples(pfd, cu, cv, pr):
    """The 16 sample coordinates (su, sv) of every pixel, ssao.comp:32-39.  The seed is uint((y * uint(display_size.y) + x) * frame_index):
    the product wraps at 2^32 (seed_thread_v masks it; the uint64 product of two numbers below 2^32 has not wrapped yet)."""
    H, W = cu.shape
    ys, xs = np.mgrid[0:H, 0:W]
    rng = seed_thread_v((ys.astype(np.uint64) * np.uint64(int(pfd["display_size"][1])) + xs.astype(np.uint64)) * np.uint64(int(pfd["frame_index"])))
    for _ in range(16):
        rng, r1 = random01_v(rng)
        rng, r2 = random01_v(rng)
        with np.errstate(invalid="ignore", over="ignore"):
            ang, dist = r1 * 2 * np.pi, r2 * pr
            yield cu + np.cos(ang) * dist, cv + np.sin(ang) * dist


def ssao(pfd, normals_bits, depth, radius=0.75):
    H, W = depth.shape
    depth = depth.astype(np.float64)
    nrm = h2f(normals_bits).astype(np.float64)
    cu, cv, cur, P, pr = _ssao_centre(pfd, depth, radius)
    Pinv = _mat(pfd, "camera_proj_inverse")
    with np.errstate(invalid="ignore"):
        N = sample_linear_repeat(nrm, cu, cv)[..., :3] @ _mat(pfd, "camera_view")[:3, :3].T
    total = np.zeros((H, W))
    for su, sv in _ssao_samples(pfd, cu, cv, pr):
        with np.errstate(invalid="ignore", over="ignore"):
            V = _unproject(Pinv, sample_linear_repeat(depth, su, sv), su, sv) - P
            total = total + _fmax((V * N).sum(-1) - 1e-4, 0.0) / ((V * V).sum(-1) + 1e-4)
    with np.errstate(invalid="ignore"):
        ao = _fmax(1.0 - (2.0 / 16.0) * total, 0.0)
    return np.where(cur == 0.0, 0.0, ao)


def ssao_sample_census(pfd, depth, radius=0.75):
    """What the 16 x W x H sample coordinates of ssao.comp reach on these inputs (pixels that return early at :17-24 take no samples).  A
    sample is counted once, by the worse of its two unnormalised coordinates t = u * W - 0.5 (v * H - 0.5):
      wrapped    -- floor(t) is finite, converts to an int and lies more than two periods from the image (t < -2 W or t >= 3 W);
      saturated  -- floor(t) is finite and at or beyond +-2^31: the float -> int conversion saturates (oracle decision xiii);
      non_finite -- t is inf or NaN: the conversion gives INT_MAX, INT_MIN or 0 and the bilinear weights are NaN."""
    H, W = depth.shape
    cu, cv, cur, _, pr = _ssao_centre(pfd, depth.astype(np.float64), radius)
    counts = dict(wrapped=0, saturated=0, non_finite=0, samples=0)
    taken = cur != 0.0
    for su, sv in _ssao_samples(pfd, cu, cv, pr):
        with np.errstate(invalid="ignore", over="ignore"):
            tx, ty = np.floor(su * W - 0.5), np.floor(sv * H - 0.5)
            bad = ~(np.isfinite(tx) & np.isfinite(ty))
            sat = ~bad & ((tx >= 2.0 ** 31) | (tx < -2.0 ** 31) | (ty >= 2.0 ** 31) | (ty < -2.0 ** 31))
            far = ~bad & ~sat & ((tx < -2 * W) | (tx >= 3 * W) | (ty < -2 * H) | (ty >= 3 * H))
        counts["wrapped"] += int((far & taken).sum())
        counts["saturated"] += int((sat & taken).sum())
        counts["non_finite"] += int((bad & taken).sum())
        counts["samples"] += int(taken.sum())
    return counts


def ssao_blur_f32(raw_bits, display_w, display_h):
    """ssao_blur.comp in fp32 with the shader's summation order (rows top to bottom, taps left to right): bit-comparable."""
    H, W = raw_bits.shape[:2]
    src = h2f(raw_bits[..., 0])
    acc = np.zeros((H, W), np.float32)
    for dy in range(-6, 7):
        for dx in range(-6, 7):
            tap, mask = _shift(src, dx, dy)
            ys, xs = np.mgrid[0:H, 0:W]
            mask &= ((xs + dx) < display_w) & ((ys + dy) < display_h)
            acc = np.where(mask, (acc + tap).astype(np.float32), acc)
    return (acc / np.float32(13.0 * 13.0)).astype(np.float32)


def ssao_blur_exact(raw_bits, display_w, display_h):
    """ssao_blur.comp:11-26 in float64: the sum of the taps inside the display (and the image), divided by 169.  The sum is EXACT whenever
    its taps are finite -- an fp16 value is a multiple of 2^-24 below 2^16, and 169 of them need 48 of float64's 53 bits -- so the only
    rounding is the division's; NaN and inf taps follow IEEE."""
    H, W = raw_bits.shape[:2]
    src = h2f(raw_bits[..., 0]).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    acc = np.zeros((H, W))
    for dy in range(-6, 7):
        for dx in range(-6, 7):
            tap, mask = _shift(src, dx, dy)
            mask &= ((xs + dx).astype(np.float32) < np.float32(display_w)) & ((ys + dy).astype(np.float32) < np.float32(display_h))
            with np.errstate(invalid="ignore"):
                acc = np.where(mask, acc + tap, acc)
    return acc / 169.0


def ssr(pfd, albedo_bgra8, normals_bits, motion_bits, depth, ray_distance=25.0, step_size=0.1, thickness=0.5, bsearch_steps=10):
    """Returns (found mask, lighting (H, W, 3), final step offset) in float64."""
    H, W = depth.shape
    depth = depth.astype(np.float64)
    nrm = h2f(normals_bits).astype(np.float64)
    mot = h2f(motion_bits).astype(np.float64)
    alb = albedo_bgra8[..., [2, 1, 0]].astype(np.float64) / 255.0
    ys, xs = np.mgrid[0:H, 0:W]
    inv = np.asarray(pfd["display_size_inverse"], np.float64)
    cu, cv = xs * inv[0], ys * inv[1]
    VPinv = _mat(pfd, "camera_viewproj_inverse")
    PV = _mat(pfd, "camera_proj") @ _mat(pfd, "camera_view")
    cam = _mat(pfd, "camera_view_inverse")[:3, 3]
    P = _unproject(VPinv, sample_linear_repeat(depth, cu, cv), cu, cv)
    N = sample_linear_repeat(nrm, cu, cv)[..., :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        I = (P - cam) / np.linalg.norm(P - cam, axis=-1, keepdims=True)
        R = I - 2.0 * (N * I).sum(-1, keepdims=True) * N
        R = R / np.linalg.norm(R, axis=-1, keepdims=True)

    def probe(offset):
        rp = P + R * offset[..., None]
        clip = np.concatenate([rp, np.ones((H, W, 1))], -1) @ PV.T
        with np.errstate(invalid="ignore", divide="ignore"):
            uv = clip[..., :2] / clip[..., 3:4] * 0.5 + 0.5
            sp = _unproject(VPinv, sample_linear_repeat(depth, uv[..., 0], uv[..., 1]), uv[..., 0], uv[..., 1])
            delta = np.linalg.norm(cam - rp, axis=-1) - np.linalg.norm(cam - sp, axis=-1)
        return delta, uv

    found = np.zeros((H, W), bool)
    prev = np.zeros((H, W))
    final = np.zeros((H, W))
    for i in range(int(np.float32(ray_distance) / np.float32(step_size))):
        off = np.full((H, W), float(np.float32(step_size) * np.float32(i)))
        with np.errstate(invalid="ignore"):
            delta, _ = probe(off)
            hit = ~found & (delta > 0.3) & (delta < thickness)
        final = np.where(hit, off, final)
        prev = np.where(~found & ~hit, off, prev)
        found |= hit
    mid = (prev + final) * 0.5
    uv = np.zeros((H, W, 2))
    for _ in range(bsearch_steps):
        with np.errstate(invalid="ignore"):
            delta, uv = probe(mid)
            inside = (delta > 0.3) & (delta < thickness)
        new_mid = np.where(inside, (prev + mid) * 0.5, mid + (mid - prev))
        prev = np.where(inside, prev, mid)
        mid = new_mid
    fu, fv = uv[..., 0], uv[..., 1]
    albedo = sample_linear_repeat(alb, fu, fv)
    with np.errstate(invalid="ignore", divide="ignore"):
        position = _unproject(VPinv, sample_linear_repeat(depth, fu, fv), fu, fv)
        mr = sample_linear_repeat(mot, fu, fv)[..., 2:4]
        V = (cam - position) / np.linalg.norm(cam - position, axis=-1, keepdims=True)
        light = pfd["directional_light"]
        L = -np.asarray(light["direction"], np.float64)[:3]
        Nl = sample_linear_repeat(nrm, fu, fv)[..., :3]
        Hh = (L + V) / np.linalg.norm(L + V, axis=-1, keepdims=True)
        metallic = np.clip(mr[..., 0:1], 0.0, 1.0)
        rough = np.clip(mr[..., 1:2], 0.04, 1.0)
        f0 = 0.04 * (1.0 - metallic) + albedo * metallic
        hv = np.fmax((Hh * V).sum(-1, keepdims=True), 0.0)
        F = f0 + (1.0 - f0) * (1.0 - hv) ** 5
        a2 = rough * rough
        nh = np.fmax((Nl * Hh).sum(-1, keepdims=True), 0.0)
        f = nh * nh * (a2 - 1.0) + 1.0
        D = a2 / (np.pi * f * f)
        k = (rough + 1.0) ** 2 * 0.125
        nv, nl = np.fmax((Nl * V).sum(-1, keepdims=True), 0.0), np.fmax((Nl * L).sum(-1, keepdims=True), 0.0)
        G = (nv / (nv * (1.0 - k) + k)) * (nl / (nl * (1.0 - k) + k))
        spec = D * G * F / np.fmax(4.0 * nv * nl, 1e-6)
        diff = (1.0 - F) * (1.0 - metallic) * albedo / np.pi
        lit = albedo * (0.2 / np.pi) + (diff + spec) * nl * np.asarray(light["intensity"], np.float64)[:3] * np.asarray(light["color"], np.float64)[:3]
    return found, np.where(found[..., None], lit, 0.0), np.where(found, final, -1.0)


# ---------------------------------------------------------------------------------------------------------
# composition.frag:60-161 in float64, written from the GLSL (and common.glsl:116-150, glsl_common.h:118-122), the presentation flip
# (pipeline.cpp:175-178) and the B8G8R8A8_SRGB store.  min / max / clamp drop a NaN operand (decision xii), the sampler is decision x / xiii.
# ---------------------------------------------------------------------------------------------------------
COMPOSITION_MUTANTS = ("ambient_times_shadow", "reflections_without_shadow", "metallic_branch_at_0.999", "roughness_floor_0", "metallic_unclamped",
                       "red_blue_swapped", "no_flip", "pcf_bias_plus", "pcf_scale_2048", "pcf_clamp", "linear_segment_to_0.04045",
                       "rg16f_read_with_rgba_stride")
SHADOW_BIAS = np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1.0]])      # common.glsl:6-11 as a math matrix
U24 = 2.0 ** -24


def srgb_code(c, slack=0.0, linear_up_to=0.0031308):
    """The B8G8R8A8_SRGB store of a float64 channel: NaN and negatives store 0, >= 1 stores 255, else the encode, * 255 + 0.5 (+ slack, in
    code units), truncated."""
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (c > 0.0) & (c < 1.0)
        x = np.where(inside, c, 0.5)
        e = np.where(x <= linear_up_to, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
        code = np.clip(np.floor(e * 255.0 + 0.5 + slack), 0, 255)
        return np.where(inside, code, np.where(c >= 1.0, 255, 0)).astype(np.uint8)


def _sample_linear_clamp(img, u, v):
    """CLAMP_TO_EDGE instead of REPEAT (the `pcf_clamp` mutant alone)."""
    H, W = img.shape[:2]
    with np.errstate(invalid="ignore"):
        fx, fy = u * W - 0.5, v * H - 0.5
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        bad = ~(np.isfinite(x0f) & np.isfinite(y0f))
        x0 = np.where(bad, 0, np.clip(x0f, -2**31, 2**31 - 1)).astype(np.int64)
        y0 = np.where(bad, 0, np.clip(y0f, -2**31, 2**31 - 1)).astype(np.int64)
    cx, cy = lambda i: np.clip(i, 0, W - 1), lambda i: np.clip(i, 0, H - 1)      # noqa: E731
    return (img[cy(y0), cx(x0)] * (1 - ax) + img[cy(y0), cx(x0 + 1)] * ax) * (1 - ay) + (img[cy(y0 + 1), cx(x0)] * (1 - ax) + img[cy(y0 + 1), cx(x0 + 1)] * ax) * ay


def _pcf(pfd, P, dist, shadow_map, mutant):
    """composition.frag:81-107.  Returns (lit taps, undecided taps, census): per pixel the number of the 16 taps that pass
    `!(sz < ds - 1e-4)` in float64, and the number whose margin |sz - (ds - 1e-4)| lies under the bound on what an fp32 evaluation of the same
    expressions may move it by ("composition cases"): such a tap may fall either way on the device."""
    sm = np.asarray(shadow_map, np.float64)
    S = sm.shape[0]
    M = SHADOW_BIAS @ _mat(pfd["directional_light"], "projview")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pl = np.concatenate([P, np.ones(P.shape[:2] + (1,))], -1) @ M.T
        s = pl[..., :3] / pl[..., 3:4]
        # fp32 error of P (|P| <= 8 m, dist >= 2 m: (16 dist + 24) u), through the matrix (4 roundings per row) and the division
        err_p = (16.0 * dist + 24.0) * U24
        mag = np.concatenate([np.abs(P), np.ones(P.shape[:2] + (1,))], -1) @ np.abs(M).T
        err_pl = np.abs(M[:, :3]).sum(1) * err_p[..., None] + 4.0 * U24 * mag
        err_s = (err_pl[..., :3] + np.abs(s) * err_pl[..., 3:4]) / np.abs(pl[..., 3:4]) + U24 * np.abs(s)
    sx, sy, sz = s[..., 0], s[..., 1], s[..., 2]
    scale = 1.0 / 2048.0 if mutant == "pcf_scale_2048" else 1.0 / 4096.0
    bias = -1e-4 if mutant == "pcf_bias_plus" else 1e-4
    sample = _sample_linear_clamp if mutant == "pcf_clamp" else sample_linear_repeat
    whole_range = float(np.nanmax(sm) - np.nanmin(sm)) if np.isfinite(sm).all() else np.inf
    lit = np.zeros(sx.shape, np.int64)
    undecided = np.zeros(sx.shape, np.int64)
    census = dict(wrapped=0, saturated=0, non_finite=0, taps=0, cleared_texel_taps=0)
    for i in range(16):
        ox, oy = ((i >> 2) - 1.5) * scale, ((i & 3) - 1.5) * scale                        # offsets[i], :89-94
        u, v = sx + ox, sy + oy
        with np.errstate(invalid="ignore", over="ignore"):
            ds = sample(sm, u, v)
            margin = sz - (ds - bias)
            lit += ~(margin < 0)
            tx, ty = np.floor(u * S - 0.5), np.floor(v * S - 0.5)
            du = S * (err_s[..., 0] + 2 * U24 * np.abs(u)) + U24 * np.abs(u * S)
            dv = S * (err_s[..., 1] + 2 * U24 * np.abs(v)) + U24 * np.abs(v * S)
            bad = ~(np.isfinite(tx) & np.isfinite(ty))
            sat = ~bad & ((np.abs(tx) >= 2.0 ** 31) | (np.abs(ty) >= 2.0 ** 31))
            far = ~bad & ~sat & ((tx < -S) | (tx >= 2 * S) | (ty < -S) | (ty >= 2 * S))
            x0 = np.mod(np.where(bad, 0, np.clip(tx, -2**31, 2**31 - 1)).astype(np.int64), S)
            y0 = np.mod(np.where(bad, 0, np.clip(ty, -2**31, 2**31 - 1)).astype(np.int64), S)
            near = np.stack([sm[(y0 + b) % S, (x0 + a) % S] for a in (-1, 0, 1, 2) for b in (-1, 0, 1, 2)], -1)
            local = near.max(-1) - near.min(-1)
            spread = np.where((du + dv) < 0.5, local, whole_range)
            err_ds = np.where(spread > 0, (du + dv) * spread, 0.0) + 8 * U24 * np.abs(near).max(-1)
            bound = err_s[..., 2] + err_ds + 2 * U24
            undecided += np.abs(margin) < bound
        census["wrapped"] += int(far.sum())
        census["saturated"] += int(sat.sum())
        census["non_finite"] += int(bad.sum())
        census["taps"] += int(bad.size)
        census["cleared_texel_taps"] += int((~bad & (near[..., 5] == 0.0)).sum())       # near[..., 5] is the texel (x0, y0)
    return lit, undecided, census


def composition(pfd, modes, albedo, normals, motion, depth, shadow_ao, reflections=None, ssao=None, shadow_map=None, mutant=None, delta=None,
                eps=0.0, code_slack=1e-3):
    """composition.frag with (shadow_mode, ambient_occlusion_mode, reflection_mode) on B8G8R8A8 albedo, RGBA16F normals / motion, D32 depth,
    RG16F or RGBA16F shadow_ao and the optional RGBA16F reflections and ssao and square D32 shadow map.  Everything returned is in the
    presented orientation (row 0 = top: G-buffer row H - 1):
      lighting   (H, W, 3) float64 r g b, before the store;      codes   (H, W, 4) uint8 b g r a, the B8G8R8A8_SRGB texels;
      pcf        under shadow_mode 1: dict(lit, undecided: (H, W) tap counts; census);
    and with `delta` (not None), the envelope an fp32 evaluation must fall into: lo, hi -- the least and the greatest lighting over the 16 sign
    combinations of moving H.V, N.L, N.H, N.V by +-delta (before their max with 0) and over the undecided PCF taps counted as dark / as lit,
    widened by the relative eps -- and code_lo, code_hi (H, W, 3) b g r: the codes of lo and hi with `code_slack` code units taken off / added.
    mutant: one of COMPOSITION_MUTANTS, a planted error."""
    assert mutant is None or mutant in COMPOSITION_MUTANTS, mutant
    H, W = depth.shape
    depth = np.asarray(depth, np.float64)
    alb = np.asarray(albedo)[..., [2, 1, 0]].astype(np.float64) / 255.0                    # :61
    ys, xs = np.mgrid[0:H, 0:W]
    cam = _mat(pfd, "camera_view_inverse")[:3, 3]
    P = _unproject(_mat(pfd, "camera_viewproj_inverse"), depth, (xs + 0.5) / W, (ys + 0.5) / H)      # :63, in_uv is the texel centre
    N = h2f(normals).astype(np.float64)[..., :3]                                           # :64
    mr = h2f(motion).astype(np.float64)[..., 2:4]                                          # :65
    sa_bits = np.asarray(shadow_ao, np.uint16)
    if mutant == "rg16f_read_with_rgba_stride" and sa_bits.shape[-1] == 2:                 # texel (x, y) read at 8 bytes a texel, wrapped into the buffer
        flat = sa_bits.reshape(-1)
        at = ((ys * W + xs) * 4) % flat.size
        sa_bits = np.stack([flat[at], flat[at + 1]], -1)
    sa = h2f(sa_bits).astype(np.float64)
    light = pfd["directional_light"]
    L = -np.asarray(light["direction"], np.float64)[:3]                                    # :74
    li, lc = np.asarray(light["intensity"], np.float64)[:3], np.asarray(light["color"], np.float64)[:3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dist = np.linalg.norm(cam - P, axis=-1)
        V = (cam - P) / dist[..., None]                                                    # :73
        Hh = (L + V) / np.linalg.norm(L + V, axis=-1, keepdims=True)                       # :75
        dots = np.stack([(Hh * V).sum(-1), (N * L).sum(-1), (N * Hh).sum(-1), (N * V).sum(-1)])
    pcf = None
    shadows = [np.ones((H, W))] * 2                                                        # (dark end, lit end)
    if modes[0] == 0:
        shadows = [sa[..., 0]] * 2
    elif modes[0] == 1:
        lit, undecided, census = _pcf(pfd, P, dist, shadow_map, mutant)
        pcf = dict(lit=lit[::-1], undecided=undecided[::-1], census=census)
        # an undecided tap that float64 saw lit may be dark on the device, and the other way round: at most `undecided` taps either way
        shadows = [np.clip(lit - undecided, 0, 16) / 16.0, np.clip(lit + undecided, 0, 16) / 16.0, lit / 16.0]
    ao = np.ones((H, W))                                                                   # :113-119
    if modes[1] == 0:
        ao = sa[..., 1]
    elif modes[1] == 1:
        ao = h2f(ssao).astype(np.float64)[..., 0]
    metallic = mr[..., 0] if mutant == "metallic_unclamped" else np.fmin(np.fmax(mr[..., 0], 0.0), 1.0)      # :122-123
    rough = np.fmin(np.fmax(mr[..., 1], 0.0 if mutant == "roughness_floor_0" else 0.04), 1.0)
    refl = h2f(reflections).astype(np.float64)[..., :3] if (modes[2] in (0, 1)) else None
    m3, r3 = metallic[..., None], rough[..., None]

    def shade(hv, nl, nh, nv, shadow):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            hv, nl, nh, nv = (np.fmax(d, 0.0) for d in (hv, nl, nh, nv))
            f0 = 0.04 * (1.0 - m3) + alb * m3                                              # :129-130
            F = f0 + (1.0 - f0) * ((1.0 - hv) ** 5)[..., None]                             # common.glsl:116-119
            a2 = rough * rough
            f = nh * nh * (a2 - 1.0) + 1.0
            D = a2 / (np.pi * f * f)                                                       # :122-127
            k = (rough + 1.0) * (rough + 1.0) * 0.125
            G = (nv / (nv * (1.0 - k) + k)) * (nl / (nl * (1.0 - k) + k))                  # :130-138
            spec_brdf = (D * G)[..., None] * F / np.fmax(4.0 * nv * nl, 1e-6)[..., None]   # :140-144
            diff_brdf = (1.0 - F) * (1.0 - m3) * alb / np.pi                               # :146-150
            sh = shadow[..., None]
            ambient = ao[..., None] * alb * (1.0 / np.pi)                                  # :135
            if mutant == "ambient_times_shadow":
                ambient = ambient * sh
            diffuse = diff_brdf * nl[..., None] * li * lc * sh                             # :136
            spec = spec_brdf * nl[..., None] * li * lc * sh                                # :137
            if refl is not None:                                                           # :139-156
                r = refl if mutant == "reflections_without_shadow" else refl * sh
                mirror = (m3 >= 0.999) if mutant == "metallic_branch_at_0.999" else (m3 == 1.0)
                spec = np.where(mirror, r, spec * (1.0 - r3) + r * r3)
            return ambient + diffuse + spec                                                # :158

    encode = (lambda c, slack=0.0: srgb_code(c, slack, 0.04045)) if mutant == "linear_segment_to_0.04045" else srgb_code      # noqa: E731
    flip = (lambda a: a) if mutant == "no_flip" else (lambda a: a[::-1])                   # noqa: E731
    lighting = shade(*dots, shadows[-1])
    order = [0, 1, 2] if mutant == "red_blue_swapped" else [2, 1, 0]
    codes = np.concatenate([encode(lighting)[..., order], np.full((H, W, 1), 255, np.uint8)], -1)
    out = dict(lighting=flip(lighting), codes=flip(codes), pcf=pcf)
    if delta is not None:
        lo, hi = lighting.copy(), lighting.copy()
        nan = np.isnan(lighting)
        for bits in range(16):
            moved = [dots[i] + (delta if bits >> i & 1 else -delta) for i in range(4)]
            for sh in shadows[:2]:
                with np.errstate(invalid="ignore"):
                    l = shade(*moved, sh)
                    lo, hi = np.fmin(lo, l), np.fmax(hi, l)
                    nan |= np.isnan(l)
        with np.errstate(invalid="ignore", over="ignore"):
            lo = np.where(lo > 0, lo * (1.0 - eps), lo * (1.0 + eps))
            hi = np.where(hi > 0, hi * (1.0 + eps), hi * (1.0 - eps))
        code_lo, code_hi = encode(lo, -code_slack)[..., ::-1], encode(hi, code_slack)[..., ::-1]
        code_lo = np.where(nan[..., ::-1], 0, code_lo)          # a NaN anywhere in the envelope: the store of a NaN (0) is admitted too
        out.update(lo=flip(lo), hi=flip(hi), code_lo=flip(code_lo), code_hi=flip(code_hi))
    return out


def raytraced_composition(raytraced_bgra8):
    """raytraced_render_path/composition.frag:11-13 with the flipped presentation and the B8G8R8A8_SRGB store: colour bytes / 255 encoded,
    alpha passed through.  Returns (codes (H, W, 4) uint8, code_lo, code_hi (H, W, 3)): the float64 encode and its +-1e-3 code-unit ends."""
    src = np.asarray(raytraced_bgra8, np.uint8)[::-1]
    c = src[..., :3].astype(np.float64) / 255.0
    codes = np.concatenate([srgb_code(c), src[..., 3:]], -1)
    return codes, srgb_code(c * (1 - 4 * U24), -1e-3), srgb_code(c * (1 + 4 * U24), 1e-3)
