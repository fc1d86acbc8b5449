/*
 * vhr_oracle.c -- TEST INFRASTRUCTURE ONLY (see vhr_oracle.h for the contract).
 *
 * Plain-C restatement of the reference's GLSL hot path.  PARITY UNPINNED (no reference
 * tests / fixtures exist; the reference cannot be built in this image).
 *
 * Decisions the reference leaves open, fixed here and mirrored,
 * independently re-implemented, by the HIP product:
 *   (i)   dispatches execute sequentially with full visibility;
 *   (ii)  svgf.comp reads the moments history from a pre-dispatch snapshot;
 *   (iii) image stores round fp32->fp16 round-to-nearest-even, loads widen exactly;
 *   (iv)  an RG16F image read as vec4 yields (r, g, 0, 1);
 *   (v)   pow(x, 128) = x^128 by seven squarings for x > 0, 0 for x <= 0;
 *   (vi)  triangle hit iff tmin < t < tmax, two-sided, Moeller-Trumbore in the op order written below, no FMA contraction (build with
 *         -ffp-contract=off), det == 0 -> miss.  A candidate whose solution is CONSISTENT -- the ray's point o + t d and the triangle's point
 *         v0 + u e1 + v e2 agree per axis to within 5e-4 + 5e-6 |coordinate|, half the padding of any box around the triangle -- is accepted as
 *         it is (it lies inside every box that leads to the triangle, in any frame: a box hierarchy cannot change the result).  For a ray within
 *         rounding of the triangle's plane the determinant is rounding noise and (t, u, v) contradict themselves: such a candidate is DECIDED
 *         AGAIN IN BINARY64 (mt_binary64: the same formulas, the same comparisons; round 6 -- round 5 rejected it, which lost true hits at
 *         grazing incidence).  The arbiter behind this rule: vhr_exact.h (the comparisons without rounding), the audit further down
 *         (orc_audit_begin), tools/audit_decision_vi.py -> profiles/r6_decision_vi.txt: of 1.6e8 exact hits on five scenes the rule rejects none,
 *         and every hit it removes is a miss in exact arithmetic.  What remains different from exact arithmetic is fp32 Moeller-Trumbore's own
 *         edge band (classes D and E of the audit), which this decision -- SURVEY.md section 8c (vi) names the formula -- keeps;
 *         closest hit = min t, ties broken by the smaller flat triangle index;
 *   (vii) sin/cos come from the 3-term Cody-Waite + Cephes-polynomial routine below,
 *         normalize(v) = v * (1 / sqrt(dot(v, v))), dot = (x*x' + y*y') + z*z';
 *   (viii) storage images are zero-initialised; int(NaN) = 0.
 */
#include "vhr_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------------------------------
 * small vector helpers (explicit op order; never contracted)
 * ---------------------------------------------------------------------------------------- */
typedef struct { float x, y, z; } v3;
typedef struct { float x, y, z, w; } v4;

static inline v3 V3(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline v3 v3add(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 v3sub(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 v3scale(v3 a, float s) { return V3(a.x * s, a.y * s, a.z * s); }
static inline v3 v3mul(v3 a, v3 b) { return V3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline v3 v3neg(v3 a) { return V3(-a.x, -a.y, -a.z); }
static inline float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static inline v3 cross3(v3 a, v3 b) {
    return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
static inline v3 normalize3(v3 a) { float inv = 1.0f / sqrtf(dot3(a, a)); return v3scale(a, inv); }

/* GLSL mat4 * vec4, column-major storage m[c*4+r]; sum accumulated left to right */
static inline v4 mat4_mul_v4(const float *m, v4 v) {
    v4 r;
    r.x = ((m[0] * v.x + m[4] * v.y) + m[8] * v.z) + m[12] * v.w;
    r.y = ((m[1] * v.x + m[5] * v.y) + m[9] * v.z) + m[13] * v.w;
    r.z = ((m[2] * v.x + m[6] * v.y) + m[10] * v.z) + m[14] * v.w;
    r.w = ((m[3] * v.x + m[7] * v.y) + m[11] * v.z) + m[15] * v.w;
    return r;
}
/* transform a point by the upper 3x4 of a column-major mat4 (w = 1) */
static inline v3 mat4_mul_point(const float *m, v3 p) {
    v3 r;
    r.x = ((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12];
    r.y = ((m[1] * p.x + m[5] * p.y) + m[9] * p.z) + m[13];
    r.z = ((m[2] * p.x + m[6] * p.y) + m[10] * p.z) + m[14];
    return r;
}

void orc_mat4_mul(const float a[16], const float b[16], float out[16]) {
    float r[16];
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 4; ++i)
            r[c * 4 + i] = ((a[0 * 4 + i] * b[c * 4 + 0] + a[1 * 4 + i] * b[c * 4 + 1]) + a[2 * 4 + i] * b[c * 4 + 2]) +
                           a[3 * 4 + i] * b[c * 4 + 3];
    memcpy(out, r, sizeof r);
}

/* general 4x4 inverse by cofactors, evaluated in double and rounded once (glm::inverse stand-in,
 * renderer.cpp:195-196) */
void orc_mat4_inverse(const float m[16], float out[16]) {
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = m[i];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    double id = (det != 0.0) ? 1.0 / det : 0.0;
    for (int i = 0; i < 16; ++i) out[i] = (float)(inv[i] * id);
}

/* src/rendering_backend/vulkan_utils.h:494-503 (column-major initialiser order) */
void orc_infinite_reverse_depth_projection(float yfov, float aspect, float znear, float out[16]) {
    float scale = 1.0f / tanf(yfov * 0.5f);
    float m[16] = { scale / aspect, 0, 0, 0, 0, scale, 0, 0, 0, 0, 0, -1.0f, 0, 0, znear, 0 };
    memcpy(out, m, sizeof m);
}

/* ------------------------------------------------------------------------------------------
 * fp16 storage semantics (decision iii)
 * ---------------------------------------------------------------------------------------- */
uint16_t orc_f32_to_f16(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    uint32_t sign = (x >> 16) & 0x8000u;
    uint32_t ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u) {                       /* inf / nan */
        if (ax > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((ax >> 13) & 0x1ffu));
        return (uint16_t)(sign | 0x7c00u);
    }
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);   /* >= 65520 rounds to inf */
    if (ax < 0x33000001u) return (uint16_t)sign;                 /* <= 2^-25 rounds to zero */
    int32_t e = (int32_t)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7fffffu) | 0x800000u;
    uint32_t shift, half;
    if (e < -14) {                                  /* subnormal half */
        shift = (uint32_t)(13 + (-14 - e));
        half = 0;
    } else {
        shift = 13;
        half = (uint32_t)(e + 15) << 10;
    }
    uint32_t mant = m >> shift;
    uint32_t rem = m & ((1u << shift) - 1u);
    uint32_t halfway = 1u << (shift - 1);
    if (e >= -14) mant &= 0x3ffu;                   /* drop implicit bit for normals */
    uint32_t h = half + mant;
    if (rem > halfway || (rem == halfway && (h & 1u))) h += 1u;  /* RTNE; carry into exponent is correct */
    return (uint16_t)(sign | h);
}

float orc_f16_to_f32(uint16_t h) {
    uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu;
    uint32_t x;
    if (e == 0) {
        if (m == 0) x = sign;
        else {
            int sh = 0;
            while (!(m & 0x400u)) { m <<= 1; ++sh; }
            m &= 0x3ffu;
            x = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | (m << 13);
        }
    } else if (e == 31) {
        x = sign | 0x7f800000u | (m << 13);
    } else {
        x = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &x, 4);
    return f;
}

static inline v4 load_rgba16f(const uint16_t *img, uint32_t W, int x, int y) {
    const uint16_t *p = img + ((size_t)y * W + (size_t)x) * 4;
    v4 r = { orc_f16_to_f32(p[0]), orc_f16_to_f32(p[1]), orc_f16_to_f32(p[2]), orc_f16_to_f32(p[3]) };
    return r;
}
/* decision (iv): RG16F read as vec4 = (r, g, 0, 1) */
static inline v4 load_rg16f(const uint16_t *img, uint32_t W, int x, int y) {
    const uint16_t *p = img + ((size_t)y * W + (size_t)x) * 2;
    v4 r = { orc_f16_to_f32(p[0]), orc_f16_to_f32(p[1]), 0.0f, 1.0f };
    return r;
}
static inline void store_rgba16f(uint16_t *img, uint32_t W, int x, int y, float a, float b, float c, float d) {
    uint16_t *p = img + ((size_t)y * W + (size_t)x) * 4;
    p[0] = orc_f32_to_f16(a); p[1] = orc_f32_to_f16(b); p[2] = orc_f32_to_f16(c); p[3] = orc_f32_to_f16(d);
}
static inline void store_rg16f(uint16_t *img, uint32_t W, int x, int y, float a, float b) {
    uint16_t *p = img + ((size_t)y * W + (size_t)x) * 2;
    p[0] = orc_f32_to_f16(a); p[1] = orc_f32_to_f16(b);
}
/* decision (viii): GLSL int(float) truncates toward zero; NaN -> 0; saturating */
static inline int f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (-2147483647 - 1);
    return (int)f;
}

/* ------------------------------------------------------------------------------------------
 * data/shaders/common.glsl
 * ---------------------------------------------------------------------------------------- */
#define ORC_TWO_PI 6.28318530717958647692528f
#define ORC_PI 3.14159265358979323846264f
#define ORC_PI_INVERSE 0.31830988618379067153776f
#define ORC_COS_PI_4 0.70710678118654752440084f

/* common.glsl:47-56 Thomas Wang hash */
uint32_t orc_seed_thread(uint32_t seed) {
    seed = (seed ^ 61u) ^ (seed >> 16);
    seed *= 9u;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2du;
    seed = seed ^ (seed >> 15);
    return seed;
}
/* common.glsl:58-64 xorshift32 */
uint32_t orc_random(uint32_t *state) {
    uint32_t s = *state;
    s ^= (s << 13);
    s ^= (s >> 17);
    s ^= (s << 5);
    *state = s;
    return s;
}
/* common.glsl:66-68 */
float orc_random01(uint32_t *state) {
    uint32_t bits = 0x3f800000u | (orc_random(state) >> 9);
    float f;
    memcpy(&f, &bits, 4);
    return f - 1.0f;
}
/* common.glsl:74-76 */
uint32_t orc_random_range(uint32_t *state, uint32_t lower, uint32_t upper) {
    return lower + (uint32_t)((float)(upper - lower + 1u) * orc_random01(state));
}

/* decision (vii): sin/cos shared definition. phi in [0, 2*pi]; quadrant reduction with a 3-term
 * Cody-Waite split of pi/2 and the Cephes sinf/cosf minimax polynomials on [-pi/4, pi/4]. */
void orc_sincos(float phi, float *s_out, float *c_out) {
    float k = rintf(phi * 0.636619772367581343f);
    float r = ((phi - k * 1.5703125f) - k * 4.837512969970703125e-4f) - k * 7.54978995489188e-8f;
    float z = r * r;
    float s = ((((-1.9515295891e-4f * z + 8.3321608736e-3f) * z + -1.6666654611e-1f) * z) * r) + r;
    float c = ((((2.443315711809948e-5f * z + -1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z) * z) + (1.0f - 0.5f * z);
    int q = ((int)k) & 3;
    float ss, cc;
    if (q == 0) { ss = s; cc = c; }
    else if (q == 1) { ss = c; cc = -s; }
    else if (q == 2) { ss = -s; cc = -c; }
    else { ss = -c; cc = s; }
    *s_out = ss;
    *c_out = cc;
}

/* common.glsl:29-34 */
static v3 uniform_sample_cone(float ux, float uy, float cos_theta_max) {
    float cos_theta = (1.0f - ux) + ux * cos_theta_max;
    float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    float phi = uy * ORC_TWO_PI;
    float s, c;
    orc_sincos(phi, &s, &c);
    return V3(c * sin_theta, s * sin_theta, cos_theta);
}
void orc_uniform_sample_cone(float u0, float u1, float cos_theta_max, float out[3]) {
    v3 r = uniform_sample_cone(u0, u1, cos_theta_max);
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
/* common.glsl:37-42 */
static v3 cosine_hemisphere(float ux, float uy) {
    float s, c;
    orc_sincos(ORC_TWO_PI * uy, &s, &c);
    float sq = sqrtf(ux);
    return V3(sq * c, sq * s, sqrtf(1.0f - ux));
}
void orc_cosine_hemisphere(float u0, float u1, float out[3]) {
    v3 r = cosine_hemisphere(u0, u1);
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

/* common.glsl:80-93 Frisvad ONB; M = three columns */
typedef struct { v3 c0, c1, c2; } m3;
static m3 onb_from_unit_vector(v3 n) {
    m3 M;
    M.c2 = n;
    if (n.z < -0.9999999f) {
        M.c0 = V3(0.0f, -1.0f, 0.0f);
        M.c1 = V3(-1.0f, 0.0f, 0.0f);
        return M;
    }
    float a = 1.0f / (1.0f + n.z);
    float b = ((-n.x) * n.y) * a;
    M.c0 = V3(1.0f - (n.x * n.x) * a, b, -n.x);
    M.c1 = V3(b, 1.0f - (n.y * n.y) * a, -n.y);
    return M;
}
void orc_onb(const float n[3], float M[9]) {
    m3 r = onb_from_unit_vector(V3(n[0], n[1], n[2]));
    M[0] = r.c0.x; M[1] = r.c0.y; M[2] = r.c0.z;
    M[3] = r.c1.x; M[4] = r.c1.y; M[5] = r.c1.z;
    M[6] = r.c2.x; M[7] = r.c2.y; M[8] = r.c2.z;
}
/* GLSL mat3 * vec3 */
static inline v3 m3_mul(m3 M, v3 v) {
    return V3((M.c0.x * v.x + M.c1.x * v.y) + M.c2.x * v.z,
              (M.c0.y * v.x + M.c1.y * v.y) + M.c2.y * v.z,
              (M.c0.z * v.x + M.c1.z * v.y) + M.c2.z * v.z);
}

static inline float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }

/* common.glsl:116-150 BRDF helpers */
static v3 fresnel_schlick(v3 f0, v3 H, v3 V) {
    float hv = fmaxf(dot3(H, V), 0.0f);
    float om = 1.0f - hv;
    float p5 = om * om * om * om * om;
    return V3(f0.x + (1.0f - f0.x) * p5, f0.y + (1.0f - f0.y) * p5, f0.z + (1.0f - f0.z) * p5);
}
static float D_GGX(float roughness, v3 N, v3 H) {
    float a2 = roughness * roughness;
    float nh = fmaxf(dot3(N, H), 0.0f);
    float f = nh * nh * (a2 - 1.0f) + 1.0f;
    return a2 / (ORC_PI * f * f);
}
static float G_GGX(float roughness, v3 N, v3 V, v3 L) {
    float k = ((roughness + 1.0f) * (roughness + 1.0f)) * 0.125f;
    float nv = fmaxf(dot3(N, V), 0.0f);
    float nl = fmaxf(dot3(N, L), 0.0f);
    float gv = nv / (nv * (1.0f - k) + k);
    float gl = nl / (nl * (1.0f - k) + k);
    return gv * gl;
}
static v3 specular_brdf(float roughness, v3 F, v3 V, v3 L, v3 N, v3 H) {
    float dg = D_GGX(roughness, N, H) * G_GGX(roughness, N, V, L);
    float denom = 4.0f * fmaxf(dot3(N, V), 0.0f) * fmaxf(dot3(N, L), 0.0f);
    float inv = 1.0f / fmaxf(denom, 1e-6f);
    return V3(dg * F.x * inv, dg * F.y * inv, dg * F.z * inv);
}
static v3 diffuse_brdf(float metallic, v3 albedo, v3 F) {
    v3 dp = V3((1.0f - F.x) * (1.0f - metallic), (1.0f - F.y) * (1.0f - metallic), (1.0f - F.z) * (1.0f - metallic));
    return V3(dp.x * albedo.x / ORC_PI, dp.y * albedo.y / ORC_PI, dp.z * albedo.z / ORC_PI);
}

/* ------------------------------------------------------------------------------------------
 * ray / triangle (decision vi)
 * ---------------------------------------------------------------------------------------- */
/* Moeller-Trumbore's comparisons (first half of decision vi); *det comes back for the audit */
static inline int mt_candidate(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float tmin, float tmax, float *t, float *u, float *v, float *det_out) {
    v3 pvec = cross3(d, e2);
    float det = dot3(e1, pvec);
    *det_out = det;
    if (det == 0.0f) return 0;
    float inv = 1.0f / det;
    v3 tvec = v3sub(o, v0);
    float uu = dot3(tvec, pvec) * inv;
    if (!(uu >= 0.0f) || uu > 1.0f) return 0;
    v3 qvec = cross3(tvec, e1);
    float vv = dot3(d, qvec) * inv;
    if (!(vv >= 0.0f) || uu + vv > 1.0f) return 0;
    float tt = dot3(e2, qvec) * inv;
    if (!(tt > tmin && tt < tmax)) return 0;
    *t = tt; *u = uu; *v = vv;
    return 1;
}
/* Second half of decision (vi), round 6: the reported point o + t d lies in the triangle's own bounding box grown by half the
 * padding of the hierarchy's boxes.  Per axis: p = fma(d, t, o); lo = v0 + min(0, e1, e2); hi = v0 + max(0, e1, e2);
 * accept iff lo - p <= tol and p - hi <= tol with tol = fma(|p|, 5e-6, 5e-4).  A NaN fails. */
static inline int hit_in_triangle_box(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float t) {
    const float o_[3] = { o.x, o.y, o.z }, d_[3] = { d.x, d.y, d.z }, v_[3] = { v0.x, v0.y, v0.z };
    const float a_[3] = { e1.x, e1.y, e1.z }, b_[3] = { e2.x, e2.y, e2.z };
    for (int i = 0; i < 3; ++i) {
        const float p = fmaf(d_[i], t, o_[i]);
        const float lo = v_[i] + fminf(0.0f, fminf(a_[i], b_[i])), hi = v_[i] + fmaxf(0.0f, fmaxf(a_[i], b_[i]));
        const float tol = fmaf(fabsf(p), 5e-6f, 5e-4f);
        if (!(lo - p <= tol && p - hi <= tol)) return 0;
    }
    return 1;
}
/* round 5's form of the second half (the ray's point against the barycentric point, 5e-4 + 5e-6 |coordinate| per axis): no longer part of
 * the decision -- the audit evaluates it beside the rule in force so that profiles/r6_decision_vi.txt can show what it cost in true hits */
static inline int hit_on_triangle_r5(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float tt, float uu, float vv) {
    const float px = o.x + d.x * tt, py = o.y + d.y * tt, pz = o.z + d.z * tt;
    const float qx = (v0.x + e1.x * uu) + e2.x * vv, qy = (v0.y + e1.y * uu) + e2.y * vv, qz = (v0.z + e1.z * uu) + e2.z * vv;
    return fabsf(px - qx) <= 5e-4f + 5e-6f * fabsf(qx) && fabsf(py - qy) <= 5e-4f + 5e-6f * fabsf(qy) && fabsf(pz - qz) <= 5e-4f + 5e-6f * fabsf(qz);
}
/* Moeller-Trumbore once more in binary64, for the pairs whose fp32 solution contradicts itself (below).  The fp32 operands are exact in
 * binary64 and so is every product of two of them; every other operation rounds once, in the order written (no contraction), and the three
 * quotients are IEEE divisions.  The comparisons are ray_triangle()'s; (t, u, v) come back rounded to fp32. */
static inline int mt_binary64(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float tmin, float tmax, float *t, float *u, float *v) {
    const double ox = o.x, oy = o.y, oz = o.z, dx = d.x, dy = d.y, dz = d.z, ax = e1.x, ay = e1.y, az = e1.z, bx = e2.x, by = e2.y, bz = e2.z;
    const double px = dy * bz - dz * by, py = dz * bx - dx * bz, pz = dx * by - dy * bx;                 /* pvec = d x e2 */
    const double det = (ax * px + ay * py) + az * pz;
    if (det == 0.0) return 0;
    const double tx = ox - (double)v0.x, ty = oy - (double)v0.y, tz = oz - (double)v0.z;                /* tvec = o - v0 */
    const double uu = ((tx * px + ty * py) + tz * pz) / det;
    if (!(uu >= 0.0) || uu > 1.0) return 0;
    const double qx = ty * az - tz * ay, qy = tz * ax - tx * az, qz = tx * ay - ty * ax;                 /* qvec = tvec x e1 */
    const double vv = ((dx * qx + dy * qy) + dz * qz) / det;
    if (!(vv >= 0.0) || uu + vv > 1.0) return 0;
    const double tt = ((bx * qx + by * qy) + bz * qz) / det;
    if (!(tt > (double)tmin && tt < (double)tmax)) return 0;
    *t = (float)tt; *u = (float)uu; *v = (float)vv;
    return 1;
}
/* Decision (vi): fp32 Moeller-Trumbore; a candidate whose solution is consistent -- the ray's point o + t d and the triangle's point
 * v0 + u e1 + v e2 agree per axis to 5e-4 + 5e-6 |coordinate|, half the padding of the hierarchy's boxes -- is accepted as it is; one whose
 * solution contradicts itself is DECIDED AGAIN IN BINARY64 (round 6; round 5 rejected it, which lost true hits at grazing incidence). */
static inline int ray_triangle(v3 o, v3 d, v3 v0, v3 e1, v3 e2, float tmin, float tmax, float *t, float *u, float *v) {
    float det;
    if (!mt_candidate(o, d, v0, e1, e2, tmin, tmax, t, u, v, &det)) return 0;
    if (hit_on_triangle_r5(o, d, v0, e1, e2, *t, *u, *v)) return 1;
    return mt_binary64(o, d, v0, e1, e2, tmin, tmax, t, u, v);
}
int orc_ray_triangle(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3],
                     float tmin, float tmax, float *t, float *u, float *v) {
    return ray_triangle(V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), V3(v0[0], v0[1], v0[2]), V3(e1[0], e1[1], e1[2]),
                        V3(e2[0], e2[1], e2[2]), tmin, tmax, t, u, v);
}

/* ------------------------------------------------------------------------------------------
 * scene: world-space triangle soup + the oracle's own (median-split) BVH
 * ---------------------------------------------------------------------------------------- */
typedef struct { v3 v0, e1, e2; uint32_t prim, tri; } orc_tri;
typedef struct { float lo[3], hi[3]; int32_t left, right; uint32_t first, count; } orc_node;
typedef struct { uint32_t w, h; int format, mag, min, au, av; uint8_t *data; } orc_texture;

struct orc_scene {
    orc_vertex *vertices; uint32_t nv;
    uint32_t *indices; uint32_t ni;
    orc_primitive *prims; uint32_t np;
    orc_tri *tris; uint32_t ntris;     /* flat order: primitive-major, triangle-minor */
    uint32_t *order;                   /* BVH leaf order -> flat triangle index */
    orc_node *nodes; uint32_t nnodes, cap_nodes;
    orc_texture *textures; uint32_t ntex;
    float srgb_lut[256];
};

static void tri_bounds(const orc_tri *t, float lo[3], float hi[3]) {
    v3 a = t->v0, b = v3add(t->v0, t->e1), c = v3add(t->v0, t->e2);
    float xs[3] = { a.x, b.x, c.x }, ys[3] = { a.y, b.y, c.y }, zs[3] = { a.z, b.z, c.z };
    lo[0] = fminf(xs[0], fminf(xs[1], xs[2])); hi[0] = fmaxf(xs[0], fmaxf(xs[1], xs[2]));
    lo[1] = fminf(ys[0], fminf(ys[1], ys[2])); hi[1] = fmaxf(ys[0], fmaxf(ys[1], ys[2]));
    lo[2] = fminf(zs[0], fminf(zs[1], zs[2])); hi[2] = fmaxf(zs[0], fmaxf(zs[1], zs[2]));
}

static int32_t build_node(orc_scene *s, float *cent, uint32_t first, uint32_t count) {
    if (s->nnodes == s->cap_nodes) {
        s->cap_nodes = s->cap_nodes ? s->cap_nodes * 2 : 1024;
        s->nodes = (orc_node *)realloc(s->nodes, sizeof(orc_node) * s->cap_nodes);
    }
    int32_t id = (int32_t)s->nnodes++;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    float clo[3] = { INFINITY, INFINITY, INFINITY }, chi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t i = first; i < first + count; ++i) {
        float tl[3], th[3];
        tri_bounds(&s->tris[s->order[i]], tl, th);
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], tl[a]); hi[a] = fmaxf(hi[a], th[a]);
            float c = cent[(size_t)s->order[i] * 3 + a];
            clo[a] = fminf(clo[a], c); chi[a] = fmaxf(chi[a], c);
        }
    }
    for (int a = 0; a < 3; ++a) {        /* conservative padding so box culling can never change a hit */
        float pad = 1e-3f + 1e-5f * fmaxf(fabsf(lo[a]), fabsf(hi[a]));
        lo[a] -= pad; hi[a] += pad;
    }
    int axis = 0;
    float ext = chi[0] - clo[0];
    if (chi[1] - clo[1] > ext) { axis = 1; ext = chi[1] - clo[1]; }
    if (chi[2] - clo[2] > ext) { axis = 2; ext = chi[2] - clo[2]; }
    orc_node n;
    memcpy(n.lo, lo, sizeof lo); memcpy(n.hi, hi, sizeof hi);
    n.left = n.right = -1; n.first = first; n.count = count;
    if (count > 4 && ext > 0.0f) {
        float split = 0.5f * (clo[axis] + chi[axis]);
        uint32_t i = first, j = first + count;
        while (i < j) {
            if (cent[(size_t)s->order[i] * 3 + axis] < split) ++i;
            else { --j; uint32_t t = s->order[i]; s->order[i] = s->order[j]; s->order[j] = t; }
        }
        uint32_t mid = i;
        if (mid == first || mid == first + count) mid = first + count / 2;
        n.count = 0;
        s->nodes[id] = n;
        int32_t l = build_node(s, cent, first, mid - first);
        int32_t r = build_node(s, cent, mid, first + count - mid);
        s->nodes[id].left = l; s->nodes[id].right = r;
    } else {
        s->nodes[id] = n;
    }
    return id;
}

orc_scene *orc_scene_create(const orc_vertex *vertices, uint32_t nv, const uint32_t *indices, uint32_t ni,
                            const orc_primitive *primitives, uint32_t np) {
    orc_scene *s = (orc_scene *)calloc(1, sizeof *s);
    s->vertices = (orc_vertex *)malloc(sizeof(orc_vertex) * (nv ? nv : 1)); memcpy(s->vertices, vertices, sizeof(orc_vertex) * nv); s->nv = nv;
    s->indices = (uint32_t *)malloc(sizeof(uint32_t) * (ni ? ni : 1)); memcpy(s->indices, indices, sizeof(uint32_t) * ni); s->ni = ni;
    s->prims = (orc_primitive *)malloc(sizeof(orc_primitive) * (np ? np : 1)); memcpy(s->prims, primitives, sizeof(orc_primitive) * np); s->np = np;
    uint32_t nt = 0;
    for (uint32_t p = 0; p < np; ++p) nt += primitives[p].index_count / 3;   /* resource_manager.cpp:637 */
    s->ntris = nt;
    s->tris = (orc_tri *)malloc(sizeof(orc_tri) * (nt ? nt : 1));
    uint32_t k = 0;
    for (uint32_t p = 0; p < np; ++p) {
        const orc_primitive *pr = &primitives[p];
        for (uint32_t t = 0; t < pr->index_count / 3; ++t) {
            /* resource_manager.cpp:638-639: indices offset by index_offset, vertices by vertex_offset;
             * :608-617: the primitive transform is baked into the geometry */
            v3 w[3];
            for (int c = 0; c < 3; ++c) {
                uint32_t vi = pr->vertex_offset + indices[pr->index_offset + 3 * t + c];
                const float *pp = vertices[vi].pos;
                w[c] = mat4_mul_point(pr->transform, V3(pp[0], pp[1], pp[2]));
            }
            s->tris[k].v0 = w[0];
            s->tris[k].e1 = v3sub(w[1], w[0]);
            s->tris[k].e2 = v3sub(w[2], w[0]);
            s->tris[k].prim = p;
            s->tris[k].tri = t;
            ++k;
        }
    }
    s->order = (uint32_t *)malloc(sizeof(uint32_t) * (nt ? nt : 1));
    float *cent = (float *)malloc(sizeof(float) * 3 * (nt ? nt : 1));
    for (uint32_t i = 0; i < nt; ++i) {
        s->order[i] = i;
        float lo[3], hi[3];
        tri_bounds(&s->tris[i], lo, hi);
        for (int a = 0; a < 3; ++a) cent[(size_t)i * 3 + a] = 0.5f * (lo[a] + hi[a]);
    }
    if (nt) build_node(s, cent, 0, nt);
    free(cent);
    for (int i = 0; i < 256; ++i) {     /* sRGB EOTF */
        double c = i / 255.0;
        s->srgb_lut[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
    return s;
}

void orc_scene_destroy(orc_scene *s) {
    if (!s) return;
    for (uint32_t i = 0; i < s->ntex; ++i) free(s->textures[i].data);
    free(s->textures); free(s->vertices); free(s->indices); free(s->prims); free(s->tris); free(s->order); free(s->nodes);
    free(s);
}

int orc_scene_add_texture(orc_scene *s, uint32_t w, uint32_t h, const uint8_t *rgba8, int format, int mag_filter,
                          int min_filter, int address_u, int address_v) {
    s->textures = (orc_texture *)realloc(s->textures, sizeof(orc_texture) * (s->ntex + 1));
    orc_texture *t = &s->textures[s->ntex];
    t->w = w; t->h = h; t->format = format; t->mag = mag_filter; t->min = min_filter; t->au = address_u; t->av = address_v;
    t->data = (uint8_t *)malloc((size_t)w * h * 4);
    memcpy(t->data, rgba8, (size_t)w * h * 4);
    return (int)s->ntex++;
}

uint32_t orc_scene_triangle_count(const orc_scene *s) { return s->ntris; }
/* the world-space records the oracle decides on, flat order: (v0, e1, e2) x ntris, and optionally each triangle's primitive */
void orc_scene_triangles(const orc_scene *s, float *v0_e1_e2, uint32_t *prim) {
    for (uint32_t i = 0; i < s->ntris; ++i) {
        const orc_tri *t = &s->tris[i];
        const float r[9] = { t->v0.x, t->v0.y, t->v0.z, t->e1.x, t->e1.y, t->e1.z, t->e2.x, t->e2.y, t->e2.z };
        memcpy(v0_e1_e2 + 9 * (size_t)i, r, sizeof r);
        if (prim) prim[i] = t->prim;
    }
}

static inline int box_hit(const orc_node *n, v3 o, v3 inv, float tmin, float tmax) {
    float t0, t1, tn = tmin, tf = tmax;
    t0 = (n->lo[0] - o.x) * inv.x; t1 = (n->hi[0] - o.x) * inv.x;
    tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
    t0 = (n->lo[1] - o.y) * inv.y; t1 = (n->hi[1] - o.y) * inv.y;
    tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
    t0 = (n->lo[2] - o.z) * inv.z; t1 = (n->hi[2] - o.z) * inv.z;
    tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
    return tn <= tf;
}

typedef struct { int hit; float t, u, v; uint32_t flat; } orc_hit;

/* ------------------------------------------------------------------------------------------
 * The audit of decision (vi) (round 6; tools/audit_decision_vi.py, tests/test_exact_arbiter.py).
 * While an audit is open, every ray that reaches trace_filtered() without the alpha test is ALSO walked in binary64 through
 * the oracle's padded boxes (a superset of what any fp32 walk visits of the triangles that matter: an exact hit point lies in
 * the unpadded box of every ancestor), and every (ray, triangle) pair met is decided three ways: fp32 Moeller-Trumbore
 * (mt_candidate), the second half of decision (vi) in its round-5 and round-6 forms, and exact arithmetic (vhr_exact.h).
 * Rules: index 0 = Moeller-Trumbore alone, 1 = round 5's residual rule (reject what contradicts itself), 2 = a candidate that was weighed and
 * dropped in round 6 (the reported point in the triangle's world-axes box: not frame-independent), 3 = the rule in force (ray_triangle():
 * what contradicts itself is decided again in binary64).
 * ---------------------------------------------------------------------------------------- */
#include "vhr_exact.h"

typedef struct {
    orc_audit_counts c;
    char pad[64];
} audit_slot;
static struct {
    int on, brute;
    uint32_t cap, nrec;
    orc_audit_record *rec;
    uint32_t log_cap, nlog;            /* the ray log (orc_audit_log_rays): every audited ray with the pixel and kind its raygen loop set */
    orc_ray_log_record *log;
    audit_slot slot[256];
} g_audit;
/* who traces: set by the raygen loop around its trace() calls, read by the ray log */
static _Thread_local uint32_t t_ray_pixel = 0xffffffffu, t_ray_kind = ORC_RAY_KIND_OTHER;

static void audit_push(const orc_audit_record *r) {
#pragma omp critical(vhr_audit_records)
    { if (g_audit.nrec < g_audit.cap) g_audit.rec[g_audit.nrec++] = *r; else g_audit.slot[0].c.records_dropped++; }
}

typedef struct { int hit; double t; uint32_t flat; } audit_best;

static void audit_pair(const orc_scene *s, uint32_t flat, v3 o, v3 d, float tmin, float tmax, int any_hit, orc_audit_counts *c,
                       int *ray_undecided, int occluded[AUD_RULES], int *exact_occluded, audit_best best[AUD_RULES], audit_best *exact_best) {
    const orc_tri *tr = &s->tris[flat];
    float t = 0, u = 0, v = 0, det = 0;
    const int mt = mt_candidate(o, d, tr->v0, tr->e1, tr->e2, tmin, tmax, &t, &u, &v, &det);
    int pass[AUD_RULES] = { mt, 0, 0, 0 };
    float tr_[AUD_RULES] = { t, t, t, t };             /* the t each rule reports */
    if (mt) {
        pass[1] = hit_on_triangle_r5(o, d, tr->v0, tr->e1, tr->e2, t, u, v);
        pass[2] = hit_in_triangle_box(o, d, tr->v0, tr->e1, tr->e2, t);
        float t3 = t, u3 = u, v3_ = v;
        pass[3] = pass[1] ? 1 : mt_binary64(o, d, tr->v0, tr->e1, tr->e2, tmin, tmax, &t3, &u3, &v3_);
        tr_[3] = t3;
        if (!pass[1]) c->escalated++;
    }
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z }, v0f[3] = { tr->v0.x, tr->v0.y, tr->v0.z };
    const float e1f[3] = { tr->e1.x, tr->e1.y, tr->e1.z }, e2f[3] = { tr->e2.x, tr->e2.y, tr->e2.z };
    const orc_exact_result ex = exact_ray_triangle(of, df, v0f, e1f, e2f, tmin, tmax);
    c->pairs++;
    char cls = 0;
    if (ex.decision < 0) { c->undecided++; *ray_undecided = 1; cls = 'U'; }
    else {
        if (ex.decision) {
            c->exact_hits++; *exact_occluded = 1;
            if (!exact_best->hit || ex.t < exact_best->t || (ex.t == exact_best->t && flat < exact_best->flat)) { exact_best->hit = 1; exact_best->t = ex.t; exact_best->flat = flat; }
        }
        if (mt) c->mt_hits++;
        if (!mt && ex.decision) { c->mt_miss_exact_hit++; cls = 'E'; }
        for (int r = 0; r < AUD_RULES; ++r) {
            if (!mt) break;
            const int k = pass[r] ? (ex.decision ? 0 : 3) : (ex.decision ? 2 : 1);      /* A, B, C, D */
            c->cls[r][k]++;
        }
        if (mt && ex.decision && !(pass[1] && pass[2] && pass[3])) cls = 'C';
        else if (mt && !ex.decision && (pass[1] || pass[2] || pass[3])) cls = 'D';
        else if (mt && !ex.decision) cls = 'B';
    }
    for (int r = 0; r < AUD_RULES; ++r) if (pass[r]) {
        occluded[r] = 1;
        const float tt_ = tr_[r];
        if (!best[r].hit || tt_ < best[r].t || ((double)tt_ == best[r].t && flat < best[r].flat)) { best[r].hit = 1; best[r].t = tt_; best[r].flat = flat; }
    }
    if (cls) {
        orc_audit_record rec;
        memset(&rec, 0, sizeof rec);
        memcpy(rec.o, of, sizeof of); memcpy(rec.d, df, sizeof df); memcpy(rec.v0, v0f, sizeof v0f); memcpy(rec.e1, e1f, sizeof e1f); memcpy(rec.e2, e2f, sizeof e2f);
        rec.tmin = tmin; rec.tmax = tmax; rec.t = t; rec.u = u; rec.v = v; rec.det = det;
        rec.xdet = ex.det; rec.xu = ex.u; rec.xv = ex.v; rec.xt = ex.t;
        rec.flat = flat; rec.mt = (uint8_t)mt; rec.pass_mask = (uint8_t)(pass[0] | pass[1] << 1 | pass[2] << 2 | pass[3] << 3);
        rec.exact = (int8_t)ex.decision; rec.any_hit = (uint8_t)any_hit; rec.cls = cls;
        audit_push(&rec);
    }
}

static inline int box_hit_f64(const orc_node *n, const double o[3], const double inv[3], double tmin, double tmax) {
    double tn = tmin, tf = tmax;
    for (int a = 0; a < 3; ++a) {
        const double t0 = ((double)n->lo[a] - o[a]) * inv[a], t1 = ((double)n->hi[a] - o[a]) * inv[a];
        tn = fmax(tn, fmin(t0, t1)); tf = fmin(tf, fmax(t0, t1));       /* a NaN (0 * inf) drops out: conservative */
    }
    return tn <= tf;
}

static void audit_ray(const orc_scene *s, v3 o, v3 d, float tmin, float tmax, int any_hit) {
    int tid = 0;
#ifdef _OPENMP
    tid = omp_get_thread_num() & 255;
#endif
    orc_audit_counts *c = &g_audit.slot[tid].c;
    if (g_audit.log) {
        orc_ray_log_record lr = { t_ray_pixel, t_ray_kind, { o.x, o.y, o.z }, tmin, { d.x, d.y, d.z }, tmax };
#pragma omp critical(vhr_audit_ray_log)
        { if (g_audit.nlog < g_audit.log_cap) g_audit.log[g_audit.nlog++] = lr; else g_audit.slot[0].c.records_dropped++; }
    }
    if (!(isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z))) { c->rays_not_finite++; return; }
    int ray_undecided = 0, exact_occluded = 0, occluded[AUD_RULES] = { 0, 0, 0, 0 };
    audit_best best[AUD_RULES] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, exact_best = { 0, 0, 0 };
    if (g_audit.brute) {
        for (uint32_t i = 0; i < s->ntris; ++i) audit_pair(s, i, o, d, tmin, tmax, any_hit, c, &ray_undecided, occluded, &exact_occluded, best, &exact_best);
    } else {
        const double od[3] = { o.x, o.y, o.z }, inv[3] = { 1.0 / (double)d.x, 1.0 / (double)d.y, 1.0 / (double)d.z };
        int32_t stack[128];
        int sp = 0;
        stack[sp++] = 0;
        while (sp) {
            const orc_node *n = &s->nodes[stack[--sp]];
            if (!box_hit_f64(n, od, inv, tmin, tmax)) continue;
            if (n->left >= 0) { stack[sp++] = n->left; stack[sp++] = n->right; continue; }
            for (uint32_t i = n->first; i < n->first + n->count; ++i)
                audit_pair(s, s->order[i], o, d, tmin, tmax, any_hit, c, &ray_undecided, occluded, &exact_occluded, best, &exact_best);
        }
    }
    c->rays[any_hit ? 0 : 1]++;
    if (ray_undecided) { c->rays_undecided++; return; }
    for (int r = 0; r < AUD_RULES; ++r) {
        if (any_hit) {
            if (!occluded[r] && exact_occluded) c->any_leak[r]++;
            if (occluded[r] && !exact_occluded) c->any_spurious[r]++;
        } else {
            if (best[r].hit != exact_best.hit) c->closest_hit_miss[r]++;
            else if (best[r].hit && best[r].flat != exact_best.flat) {
                c->closest_differs[r]++;
                if (fabs(best[r].t - exact_best.t) > 1e-4 * fmax(1.0, fabs(exact_best.t))) c->closest_differs_far[r]++;
            }
        }
    }
}

void orc_audit_begin(int brute_force, uint32_t max_records) {
    memset(&g_audit, 0, sizeof g_audit);
    g_audit.brute = brute_force;
    g_audit.cap = max_records;
    g_audit.rec = (orc_audit_record *)malloc(sizeof(orc_audit_record) * (max_records ? max_records : 1));
    g_audit.on = 1;
}
void orc_audit_log_rays(uint32_t max_rays) {
    g_audit.log = (orc_ray_log_record *)malloc(sizeof(orc_ray_log_record) * (max_rays ? max_rays : 1));
    g_audit.log_cap = max_rays;
    g_audit.nlog = 0;
}
uint32_t orc_audit_ray_log(orc_ray_log_record *out) {
    if (out && g_audit.log) memcpy(out, g_audit.log, sizeof(orc_ray_log_record) * g_audit.nlog);
    return g_audit.nlog;
}
uint32_t orc_audit_end(orc_audit_counts *out, orc_audit_record *records) {
    g_audit.on = 0;
    free(g_audit.log);
    g_audit.log = NULL;
    orc_audit_counts sum;
    memset(&sum, 0, sizeof sum);
    for (int i = 0; i < 256; ++i) {
        const uint64_t *a = (const uint64_t *)&g_audit.slot[i].c;
        uint64_t *b = (uint64_t *)&sum;
        for (size_t k = 0; k < sizeof(orc_audit_counts) / sizeof(uint64_t); ++k) b[k] += a[k];
    }
    if (out) *out = sum;
    if (records) memcpy(records, g_audit.rec, sizeof(orc_audit_record) * g_audit.nrec);
    free(g_audit.rec);
    g_audit.rec = NULL;
    return g_audit.nrec;
}
int orc_ray_triangle_exact(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3], float tmin, float tmax,
                           double out_det_u_v_t[4]) {
    const orc_exact_result r = exact_ray_triangle(o, d, v0, e1, e2, tmin, tmax);
    if (out_det_u_v_t) { out_det_u_v_t[0] = r.det; out_det_u_v_t[1] = r.u; out_det_u_v_t[2] = r.v; out_det_u_v_t[3] = r.t; }
    return r.decision;
}
/* the three fp32 decisions of one pair, for the known-answer tests: bit 0 Moeller-Trumbore's comparisons, bit 1 round 5's rule, bit 2 the box rule, bit 3 the rule in force */
int orc_ray_triangle_rules(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3], float tmin, float tmax,
                           float out_t_u_v_det[4]) {
    float t = 0, u = 0, v = 0, det = 0;
    const v3 O = V3(o[0], o[1], o[2]), D = V3(d[0], d[1], d[2]), A = V3(v0[0], v0[1], v0[2]), E1 = V3(e1[0], e1[1], e1[2]), E2 = V3(e2[0], e2[1], e2[2]);
    const int mt = mt_candidate(O, D, A, E1, E2, tmin, tmax, &t, &u, &v, &det);
    if (out_t_u_v_det) { out_t_u_v_det[0] = t; out_t_u_v_det[1] = u; out_t_u_v_det[2] = v; out_t_u_v_det[3] = det; }
    if (!mt) return 0;
    const int r5 = hit_on_triangle_r5(O, D, A, E1, E2, t, u, v);
    float t3 = t, u3 = u, v3_ = v;
    const int r6 = r5 ? 1 : mt_binary64(O, D, A, E1, E2, tmin, tmax, &t3, &u3, &v3_);
    return 1 | r5 << 1 | hit_in_triangle_box(O, D, A, E1, E2, t) << 2 | r6 << 3;
}

/* ------------------------------------------------------------------------------------------
 * Per-ray exact truth (tests/ray_truth.py, tests/test_ray_truth.py, tests/test_gpu_ray_truth.py): every triangle of the scene against
 * every ray of a batch with exact_ray_triangle() -- no boxes, so the answer owes nothing to any hierarchy -- and, per ray, the pairs that
 * matter to a verdict on somebody's answer: every exact hit, every pair the binary64 filter leaves undecided (python Fractions settle
 * them), and every exact miss inside fp32 Moeller-Trumbore's forward error band (margin <= 1).  Bounds and margin are
 * tests/ray_truth.py's mt_error_margin() restated operation by operation (tests/test_ray_truth.py holds the two equal): k = 8 * 2^-24,
 *      eu = k (P(un) + |u| P(det)) / |det|, ev, et alike with the permanents P of vhr_exact.h,
 *      margin = min(|u|/eu, |1-u|/eu, |v|/ev, |1-u-v|/(eu+ev+2^-24), |t-tmin|/et, |tmax-t|/et).
 * (tests/ray_truth.py then narrows the band misses to those whose numerators allow an fp32 hit at all: numerators_allow_a_hit.)
 * A determinant that is CERTAINLY 0 (every term of it is exactly 0: a degenerate triangle, a ray along an axis in an axis-aligned
 * plane) is 0 in fp32 as well -- products and sums of zeros -- so such a pair is a miss for everybody and is not returned.
 * prim_masks (optional, one per primitive) with ray_masks (optional, one per ray) and cull_mask: ray i carries cull_mask & ray_masks[i],
 * and a primitive whose mask shares no bit with it does not exist for that ray.
 * Two calls: pairs == NULL counts (offsets[0..n] out, returns the total); then with room for that many pairs (offsets in). */
static inline void truth_bounds(const float of[3], const float df[3], const float v0f[3], const float e1f[3], const float e2f[3],
                                float tminf, float tmaxf, const orc_exact_result *ex, double *eu, double *ev, double *et, double *margin) {
    double tv[3], ad[3], a1[3], a2[3], ppv[3], pqv[3];
    for (int i = 0; i < 3; ++i) { tv[i] = fabs((double)of[i]) + fabs((double)v0f[i]); ad[i] = fabs((double)df[i]); a1[i] = fabs((double)e1f[i]); a2[i] = fabs((double)e2f[i]); }
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        ppv[i] = ad[j] * a2[k] + ad[k] * a2[j];
        pqv[i] = tv[j] * a1[k] + tv[k] * a1[j];
    }
    const double pdet = (a1[0] * ppv[0] + a1[1] * ppv[1]) + a1[2] * ppv[2];
    const double pun = (tv[0] * ppv[0] + tv[1] * ppv[1]) + tv[2] * ppv[2];
    const double pvn = (ad[0] * pqv[0] + ad[1] * pqv[1]) + ad[2] * pqv[2];
    const double ptn = (a2[0] * pqv[0] + a2[1] * pqv[1]) + a2[2] * pqv[2];
    const double det = fabs(ex->det);
    if (det == 0.0) { *eu = *ev = *et = INFINITY; *margin = 0.0; return; }
    const double eps = 0x1p-24, k = 8.0 * eps, u = ex->u, v = ex->v, t = ex->t;
    *eu = k * (pun + fabs(u) * pdet) / det;
    *ev = k * (pvn + fabs(v) * pdet) / det;
    *et = k * (ptn + fabs(t) * pdet) / det;
    const double m[6] = { fabs(u) / *eu, fabs(1.0 - u) / *eu, fabs(v) / *ev, fabs((1.0 - u) - v) / ((*eu + *ev) + eps),
                          fabs(t - (double)tminf) / *et, fabs((double)tmaxf - t) / *et };
    double best = m[0];
    for (int i = 1; i < 6; ++i) if (m[i] < best) best = m[i];
    *margin = best;
}

/* one pair: the exact decision, (det, u, v, t), the bounds (eu, ev, et) and the margin as orc_ray_truth computes them */
int orc_ray_triangle_bounds(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3], float tmin, float tmax,
                            double out_det_u_v_t_eu_ev_et_margin[8]) {
    const orc_exact_result ex = exact_ray_triangle(o, d, v0, e1, e2, tmin, tmax);
    double *q = out_det_u_v_t_eu_ev_et_margin;
    q[0] = ex.det; q[1] = ex.u; q[2] = ex.v; q[3] = ex.t;
    truth_bounds(o, d, v0, e1, e2, tmin, tmax, &ex, &q[4], &q[5], &q[6], &q[7]);
    return ex.decision;
}

uint64_t orc_ray_truth(const orc_scene *s, const float *rays, uint32_t n_rays, const uint8_t *prim_masks, const uint8_t *ray_masks,
                       uint32_t cull_mask, uint64_t *offsets, orc_truth_pair *pairs) {
    const int count_only = pairs == NULL;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t r = 0; r < (int64_t)n_rays; ++r) {
        const float *ray = rays + 8 * r;
        const float of[3] = { ray[0], ray[1], ray[2] }, df[3] = { ray[4], ray[5], ray[6] }, tmin = ray[3], tmax = ray[7];
        const uint32_t rmask = cull_mask & (ray_masks ? ray_masks[r] : 0xffu);
        uint64_t k = 0;
        orc_truth_pair *out = count_only ? NULL : pairs + offsets[r];
        for (uint32_t i = 0; i < s->ntris; ++i) {
            const orc_tri *tr = &s->tris[i];
            if (prim_masks && !(prim_masks[tr->prim] & rmask)) continue;
            const float v0f[3] = { tr->v0.x, tr->v0.y, tr->v0.z }, e1f[3] = { tr->e1.x, tr->e1.y, tr->e1.z }, e2f[3] = { tr->e2.x, tr->e2.y, tr->e2.z };
            const orc_exact_result ex = exact_ray_triangle(of, df, v0f, e1f, e2f, tmin, tmax);
            if (!isfinite(ex.det)) continue;                         /* a ray with a NaN or an infinity in it: a miss for everybody */
            if (ex.decision == 0 && ex.det == 0.0) continue;         /* certainly 0 (a cancellation to 0 comes back undecided) */
            double eu = 0, ev = 0, et = 0, margin = INFINITY;
            truth_bounds(of, df, v0f, e1f, e2f, tmin, tmax, &ex, &eu, &ev, &et, &margin);
            if (ex.decision == 0 && !(margin <= 1.0)) continue;
            if (!count_only) {
                orc_truth_pair *p = &out[k];
                p->flat = i; p->decision = ex.decision; p->det = ex.det; p->u = ex.u; p->v = ex.v; p->t = ex.t;
                p->eu = eu; p->ev = ev; p->et = et; p->margin = margin;
            }
            ++k;
        }
        if (count_only) offsets[r + 1] = k;
    }
    if (count_only) {
        offsets[0] = 0;
        for (uint32_t r = 0; r < n_rays; ++r) offsets[r + 1] += offsets[r];
    }
    return offsets[n_rays];
}

/* any_hit != 0: return on the first accepted triangle (gl_RayFlagsTerminateOnFirstHitEXT,
 * raygen.rgen:39); otherwise closest hit with the flat-index tie break (decision vi) */
/* alpha_test != 0: every candidate first runs shadow_anyhit.rahit (rays traced with gl_RayFlagsNoOpaqueEXT by the
 * raytraced render path, raygen_test_alpha.rgen:20 / closesthit_test_alpha.rchit:42); an ignored candidate does not exist */
static int alpha_ignored(const orc_scene *s, uint32_t flat, float u, float v);
static orc_hit trace_filtered(const orc_scene *s, v3 o, v3 d, float tmin, float tmax, int any_hit, int use_bvh, int alpha_test) {
    orc_hit best = { 0, tmax, 0, 0, 0xffffffffu };
    if (s->ntris == 0) return best;
    if (g_audit.on && !alpha_test) audit_ray(s, o, d, tmin, tmax, any_hit);
    if (!use_bvh) {
        for (uint32_t i = 0; i < s->ntris; ++i) {
            const orc_tri *tr = &s->tris[i];
            float t, u, v;
            if (ray_triangle(o, d, tr->v0, tr->e1, tr->e2, tmin, tmax, &t, &u, &v)) {
                if (alpha_test && alpha_ignored(s, i, u, v)) continue;
                if (any_hit) { best.hit = 1; best.t = t; best.u = u; best.v = v; best.flat = i; return best; }
                if (!best.hit || t < best.t || (t == best.t && i < best.flat)) { best.hit = 1; best.t = t; best.u = u; best.v = v; best.flat = i; }
            }
        }
        return best;
    }
    v3 inv = V3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    int32_t stack[128];
    int sp = 0;
    stack[sp++] = 0;
    while (sp) {
        const orc_node *n = &s->nodes[stack[--sp]];
        /* closest hit keeps the full [tmin, tmax] interval on purpose: pruning by best.t would be an
         * optimisation whose only effect must be none */
        if (!box_hit(n, o, inv, tmin, tmax)) continue;
        if (n->left >= 0) { stack[sp++] = n->left; stack[sp++] = n->right; continue; }
        for (uint32_t i = n->first; i < n->first + n->count; ++i) {
            uint32_t flat = s->order[i];
            const orc_tri *tr = &s->tris[flat];
            float t, u, v;
            if (ray_triangle(o, d, tr->v0, tr->e1, tr->e2, tmin, tmax, &t, &u, &v)) {
                if (alpha_test && alpha_ignored(s, flat, u, v)) continue;
                if (any_hit) { best.hit = 1; best.t = t; best.u = u; best.v = v; best.flat = flat; return best; }
                if (!best.hit || t < best.t || (t == best.t && flat < best.flat)) { best.hit = 1; best.t = t; best.u = u; best.v = v; best.flat = flat; }
            }
        }
    }
    return best;
}
static orc_hit trace(const orc_scene *s, v3 o, v3 d, float tmin, float tmax, int any_hit, int use_bvh) {
    return trace_filtered(s, o, d, tmin, tmax, any_hit, use_bvh, 0);        /* all-opaque geometry, resource_manager.cpp:633 */
}

int orc_scene_occluded(const orc_scene *s, const float o[3], const float d[3], float tmin, float tmax, int use_bvh) {
    return trace(s, V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), tmin, tmax, 1, use_bvh).hit;
}
int orc_scene_closest(const orc_scene *s, const float o[3], const float d[3], float tmin, float tmax, int use_bvh,
                      float *t, float *u, float *v, uint32_t *prim, uint32_t *tri_in_prim) {
    orc_hit h = trace(s, V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), tmin, tmax, 0, use_bvh);
    if (!h.hit) return 0;
    *t = h.t; *u = h.u; *v = h.v; *prim = s->tris[h.flat].prim; *tri_in_prim = s->tris[h.flat].tri;
    return 1;
}

/* ------------------------------------------------------------------------------------------
 * texture(): LOD 0, per-texture sampler (resource_manager.cpp:58-69,152-196; scene_loader.cpp:241-300)
 * ---------------------------------------------------------------------------------------- */
static inline int wrap_coord(int i, int n, int mode) {
    if (mode == 2) return i < 0 ? 0 : (i >= n ? n - 1 : i);              /* CLAMP_TO_EDGE */
    if (mode == 1) {                                                       /* MIRRORED_REPEAT */
        int p = 2 * n;
        int m = i % p; if (m < 0) m += p;
        return m < n ? m : p - 1 - m;
    }
    int m = i % n; if (m < 0) m += n;                                      /* REPEAT */
    return m;
}
static inline v4 texel(const orc_scene *s, const orc_texture *t, int x, int y) {
    const uint8_t *p = t->data + ((size_t)y * t->w + (size_t)x) * 4;
    v4 r;
    if (t->format == 43) { r.x = s->srgb_lut[p[0]]; r.y = s->srgb_lut[p[1]]; r.z = s->srgb_lut[p[2]]; }
    else { r.x = p[0] * (1.0f / 255.0f); r.y = p[1] * (1.0f / 255.0f); r.z = p[2] * (1.0f / 255.0f); }
    r.w = p[3] * (1.0f / 255.0f);
    return r;
}
static v4 sample_texture(const orc_scene *s, int idx, float u, float v) {
    v4 zero = { 0, 0, 0, 0 };
    if (idx < 0 || (uint32_t)idx >= s->ntex) return zero;
    const orc_texture *t = &s->textures[idx];
    float x = u * (float)t->w, y = v * (float)t->h;
    if (t->mag == 0) {
        int ix = wrap_coord((int)floorf(x), (int)t->w, t->au), iy = wrap_coord((int)floorf(y), (int)t->h, t->av);
        return texel(s, t, ix, iy);
    }
    x -= 0.5f; y -= 0.5f;
    float fx0 = floorf(x), fy0 = floorf(y);
    float fx = x - fx0, fy = y - fy0;
    int x0 = wrap_coord((int)fx0, (int)t->w, t->au), x1 = wrap_coord((int)fx0 + 1, (int)t->w, t->au);
    int y0 = wrap_coord((int)fy0, (int)t->h, t->av), y1 = wrap_coord((int)fy0 + 1, (int)t->h, t->av);
    v4 a = texel(s, t, x0, y0), b = texel(s, t, x1, y0), c = texel(s, t, x0, y1), d = texel(s, t, x1, y1);
    v4 r;
    r.x = (a.x * (1.0f - fx) + b.x * fx) * (1.0f - fy) + (c.x * (1.0f - fx) + d.x * fx) * fy;
    r.y = (a.y * (1.0f - fx) + b.y * fx) * (1.0f - fy) + (c.y * (1.0f - fx) + d.y * fx) * fy;
    r.z = (a.z * (1.0f - fx) + b.z * fx) * (1.0f - fy) + (c.z * (1.0f - fx) + d.z * fx) * fy;
    r.w = (a.w * (1.0f - fx) + b.w * fx) * (1.0f - fy) + (c.w * (1.0f - fx) + d.w * fx) * fy;
    return r;
}

/* ------------------------------------------------------------------------------------------
 * reflection_hit.rchit:10-72 (closest-hit shading); returns the payload rgb, a = 1
 * ---------------------------------------------------------------------------------------- */
/* second_bounce (may be NULL): the documented 2-bounce extension (BASELINE config 5; the reference traces one bounce and
 * declares recursion depth 2, pipeline.cpp:285).  When given, *second_bounce is the payload of a mirror ray traced from this
 * hit and it replaces / blends into the specular term exactly like composition.frag:141-149 blends the first bounce at
 * the primary hit: metallic == 1 ? reflections : mix(specular_lighting, reflections, roughness).  hit_position / hit_normal
 * (optional) return the world-space hit point and the shader's N for the caller to build that ray. */
static v4 reflection_hit_ex(const orc_scene *s, const orc_per_frame_data *pfd, const orc_hit *h, const v4 *second_bounce,
                            v3 *hit_position, v3 *hit_normal) {
    const orc_tri *tr = &s->tris[h->flat];
    const orc_primitive *prim = &s->prims[tr->prim];                               /* :11 gl_GeometryIndexEXT */
    uint32_t i0 = s->indices[prim->index_offset + 3 * tr->tri + 0];               /* :13-15 gl_PrimitiveID */
    uint32_t i1 = s->indices[prim->index_offset + 3 * tr->tri + 1];
    uint32_t i2 = s->indices[prim->index_offset + 3 * tr->tri + 2];
    const orc_vertex *a = &s->vertices[prim->vertex_offset + i0];                 /* :17-19 */
    const orc_vertex *b = &s->vertices[prim->vertex_offset + i1];
    const orc_vertex *c = &s->vertices[prim->vertex_offset + i2];
    float bx = 1.0f - h->u - h->v, by = h->u, bz = h->v;                          /* :21 */
    float uvx = a->uv0[0] * bx + b->uv0[0] * by + c->uv0[0] * bz;                 /* :22 */
    float uvy = a->uv0[1] * bx + b->uv0[1] * by + c->uv0[1] * bz;
    v3 normal = V3(a->normal[0] * bx + b->normal[0] * by + c->normal[0] * bz,     /* :23 object space, unnormalised */
                   a->normal[1] * bx + b->normal[1] * by + c->normal[1] * bz,
                   a->normal[2] * bx + b->normal[2] * by + c->normal[2] * bz);
    v3 opos = V3(a->pos[0] * bx + b->pos[0] * by + c->pos[0] * bz,
                 a->pos[1] * bx + b->pos[1] * by + c->pos[1] * bz,
                 a->pos[2] * bx + b->pos[2] * by + c->pos[2] * bz);
    v3 position = mat4_mul_point(prim->transform, opos);                           /* :24 */

    v3 albedo;
    if (prim->material.base_color_texture == -1)                                   /* :27-32 */
        albedo = V3(prim->material.base_color[0], prim->material.base_color[1], prim->material.base_color[2]);
    else { v4 t = sample_texture(s, prim->material.base_color_texture, uvx, uvy); albedo = V3(t.x, t.y, t.z); }
    float metallic = prim->material.metallic_factor;                               /* :33-39 */
    float roughness = prim->material.roughness_factor;
    if (prim->material.metallic_roughness_texture != -1) {
        v4 mr = sample_texture(s, prim->material.metallic_roughness_texture, uvx, uvy);
        metallic *= mr.y;
        roughness *= mr.z;
    }
    v3 cam = V3(pfd->camera_view_inverse[12], pfd->camera_view_inverse[13], pfd->camera_view_inverse[14]);   /* :41 */
    v3 V = normalize3(v3sub(cam, position));
    v3 L = v3neg(V3(pfd->directional_light.direction[0], pfd->directional_light.direction[1], pfd->directional_light.direction[2]));
    v3 N = normal;
    v3 H = normalize3(v3add(L, V));
    roughness = fminf(fmaxf(roughness, 0.04f), 1.0f);                              /* :53-55 */
    metallic = fminf(fmaxf(metallic, 0.0f), 1.0f);
    float ambient_factor = ORC_PI_INVERSE * 0.2f;                                  /* :59 */
    v3 li = V3(pfd->directional_light.intensity[0], pfd->directional_light.intensity[1], pfd->directional_light.intensity[2]);
    v3 lc = V3(pfd->directional_light.color[0], pfd->directional_light.color[1], pfd->directional_light.color[2]);
    v3 f0 = V3(0.04f * (1.0f - metallic) + albedo.x * metallic, 0.04f * (1.0f - metallic) + albedo.y * metallic,
               0.04f * (1.0f - metallic) + albedo.z * metallic);                   /* :63-64 mix */
    v3 F = fresnel_schlick(f0, H, V);
    v3 ambient = v3scale(albedo, ambient_factor);                                  /* :67 */
    v3 diffuse = diffuse_brdf(metallic, albedo, F);
    v3 specular = specular_brdf(roughness, F, V, L, N, H);
    float nl = fmaxf(dot3(N, L), 0.0f);
    if (hit_position) *hit_position = position;
    if (hit_normal) *hit_normal = N;
    if (second_bounce) {
        v3 dl = v3mul(v3mul(v3scale(diffuse, nl), li), lc);                        /* composition.frag:138 without the shadow factor */
        v3 sl = v3mul(v3mul(v3scale(specular, nl), li), lc);                       /* :139 */
        v3 refl = V3(second_bounce->x, second_bounce->y, second_bounce->z);
        if (metallic == 1.0f) sl = refl;                                           /* :141-149 */
        else sl = V3(mixf(sl.x, refl.x, roughness), mixf(sl.y, refl.y, roughness), mixf(sl.z, refl.z, roughness));
        v3 lighting2 = v3add(v3add(ambient, dl), sl);                              /* :160 */
        v4 r2 = { lighting2.x, lighting2.y, lighting2.z, 1.0f };
        return r2;
    }
    v3 lit = v3mul(v3mul(v3scale(v3add(diffuse, specular), nl), li), lc);          /* :70 */
    v3 lighting = v3add(ambient, lit);
    v4 r = { lighting.x, lighting.y, lighting.z, 1.0f };
    return r;
}
static v4 reflection_hit(const orc_scene *s, const orc_per_frame_data *pfd, const orc_hit *h) {
    return reflection_hit_ex(s, pfd, h, NULL, NULL, NULL);
}

/* ------------------------------------------------------------------------------------------
 * raygen.rgen:14-66 (+ miss.rmiss:6-8, reflection_miss.rmiss:6-8)
 * ---------------------------------------------------------------------------------------- */
void orc_default_trace_params(orc_trace_params *p) {
    p->shadow_enable = 1; p->ao_spp = 2; p->ao_tmax = 5.0f; p->reflections = 1;
    p->cone_cos_max = 0.999995f; p->normal_bias = 0.1f; p->tmin = 0.01f; p->tmax = 10000.0f;
}

/* glsl_common.h:118-122 */
static v3 get_world_space_position(const orc_per_frame_data *pfd, float depth, float u, float v) {
    v4 ndc = { u * 2.0f - 1.0f, v * 2.0f - 1.0f, depth, 1.0f };
    v4 r = mat4_mul_v4(pfd->camera_viewproj_inverse, ndc);
    return V3(r.x / r.w, r.y / r.w, r.z / r.w);
}

void orc_raygen(const orc_scene *s, const orc_per_frame_data *pfd, const orc_trace_params *tp, uint32_t W, uint32_t H,
                uint32_t row_begin, uint32_t row_end, const uint16_t *normals_ids, const float *depth,
                uint16_t *shadow_ao, uint16_t *reflections, uint8_t *vis_mask, uint64_t *rays_out, int use_bvh) {
    uint64_t rays = 0;
#pragma omp parallel for schedule(dynamic, 2) reduction(+ : rays)
    for (int64_t yy = (int64_t)row_begin; yy < (int64_t)row_end; ++yy) {
        uint32_t y = (uint32_t)yy;
        for (uint32_t x = 0; x < W; ++x) {
            float u = ((float)x + 0.5f) / (float)W;                                       /* :15-16 */
            float v = ((float)y + 0.5f) / (float)H;
            uint32_t rng = orc_seed_thread((y * H + x) * pfd->frame_index);               /* :17 LaunchSize.y quirk */
            float d = depth[(size_t)y * W + x];                                           /* :19 texel-centre fetch */
            uint8_t mask = 0;
            if (d == 0.0f) {                                                              /* :20-24 */
                store_rg16f(shadow_ao, W, (int)x, (int)y, 1.0f, 1.0f);
                if (reflections) store_rgba16f(reflections, W, (int)x, (int)y, 0, 0, 0, 0);
                if (vis_mask) vis_mask[(size_t)y * W + x] = 0x40;
                continue;
            }
            t_ray_pixel = y * W + x;
            v3 P = get_world_space_position(pfd, d, u, v);                                /* :26 */
            v3 L = v3neg(V3(pfd->directional_light.direction[0], pfd->directional_light.direction[1],
                            pfd->directional_light.direction[2]));                        /* :27 */
            v4 nid = load_rgba16f(normals_ids, W, (int)x, (int)y);                        /* :28 */
            v3 N = V3(nid.x, nid.y, nid.z);
            v3 origin = v3add(P, v3scale(N, tp->normal_bias));                            /* :29 */

            float rnd1 = orc_random01(&rng);                                              /* :32-33 */
            float rnd2 = orc_random01(&rng);
            float shadow_payload = 1.0f;
            if (tp->shadow_enable) {
                v3 cone_dir = normalize3(uniform_sample_cone(rnd1, rnd2, tp->cone_cos_max));   /* :34 */
                m3 R = onb_from_unit_vector(L);                                           /* :35 */
                v3 dir = m3_mul(R, cone_dir);
                /* :37-41 four identical traces; the payload of the last one survives == one trace */
                t_ray_kind = ORC_RAY_KIND_SHADOW;
                int occluded = trace(s, origin, dir, tp->tmin, tp->tmax, 1, use_bvh).hit;
                shadow_payload = occluded ? 0.0f : 1.0f;                                  /* miss.rmiss:7 */
                ++rays;
            }
            if (shadow_payload != 0.0f) mask |= 1;

            float ao_payload = 0.0f;                                                      /* :44-55 */
            for (uint32_t i = 0; i < tp->ao_spp; ++i) {
                rnd1 = orc_random01(&rng);
                rnd2 = orc_random01(&rng);
                v3 rnd_dir = cosine_hemisphere(rnd1, rnd2);
                m3 R = onb_from_unit_vector(N);
                v3 dir = m3_mul(R, rnd_dir);
                t_ray_kind = ORC_RAY_KIND_AO;
                int occluded = trace(s, origin, dir, tp->tmin, tp->ao_tmax, 1, use_bvh).hit;
                ao_payload += occluded ? 0.0f : 1.0f;
                if (!occluded && i < 5) mask |= (uint8_t)(2u << i);
                ++rays;
            }
            if (tp->ao_spp) ao_payload /= (float)tp->ao_spp; else ao_payload = 1.0f;
            store_rg16f(shadow_ao, W, (int)x, (int)y, shadow_payload, ao_payload);       /* :57 (RG16F target) */

            if (reflections) {
                v4 payload = { 0, 0, 0, 0 };
                if (tp->reflections) {                                                    /* :60-65 */
                    v3 cam = V3(pfd->camera_view_inverse[12], pfd->camera_view_inverse[13], pfd->camera_view_inverse[14]);
                    v3 I = normalize3(v3sub(P, cam));
                    float ni2 = 2.0f * dot3(N, I);
                    v3 rdir = v3sub(I, v3scale(N, ni2));                                   /* reflect(I, N) */
                    t_ray_kind = ORC_RAY_KIND_MIRROR;
                    orc_hit h = trace(s, origin, rdir, tp->tmin, tp->tmax, 0, use_bvh);
                    ++rays;
                    if (h.hit && tp->reflections >= 2) {
                        /* 2-bounce extension: a mirror ray from the first hit, about the shader's N (normalised, facing the
                         * incoming ray), origin biased like raygen.rgen:29, shaded by reflection_hit.rchit without recursion */
                        v3 hp, hn;
                        (void)reflection_hit_ex(s, pfd, &h, NULL, &hp, &hn);
                        v3 nn = normalize3(hn);
                        float ni = dot3(nn, rdir);
                        v3 nf = ni < 0.0f ? nn : v3neg(nn);
                        v3 d2 = v3sub(rdir, v3scale(nn, 2.0f * ni));
                        v3 o2 = v3add(hp, v3scale(nf, tp->normal_bias));
                        t_ray_kind = ORC_RAY_KIND_SECOND_BOUNCE;
                        orc_hit h2 = trace(s, o2, d2, tp->tmin, tp->tmax, 0, use_bvh);
                        ++rays;
                        v4 second = { 0, 0, 0, 0 };                                        /* reflection_miss.rmiss:7 */
                        if (h2.hit) second = reflection_hit(s, pfd, &h2);
                        payload = reflection_hit_ex(s, pfd, &h, &second, NULL, NULL);
                        mask |= 0x80;
                    } else
                    if (h.hit) { payload = reflection_hit(s, pfd, &h); mask |= 0x80; }     /* else reflection_miss.rmiss:7 */
                }
                store_rgba16f(reflections, W, (int)x, (int)y, payload.x, payload.y, payload.z, payload.w);
            }
            if (vis_mask) vis_mask[(size_t)y * W + x] = mask;
            t_ray_pixel = 0xffffffffu; t_ray_kind = ORC_RAY_KIND_OTHER;
        }
    }
    if (rays_out) *rays_out = rays;
}

/* ------------------------------------------------------------------------------------------
 * next row f4: the raytraced render path (raytraced_render_path.cpp:11-76)
 *   raytraced_render_path/raygen.rgen:10-23, raygen_test_alpha.rgen:10-23, miss.rmiss:6-8, shadow_miss.rmiss:6-8,
 *   closesthit.rchit:10-58, closesthit_test_alpha.rchit:10-51, shadow_anyhit.rahit:8-27, composition.frag:11-13
 * Decision (ix): `textures[-1]` (a primitive without a base colour texture, sampled unconditionally by
 * shadow_anyhit.rahit:23 and closesthit_test_alpha.rchit:26) is out of bounds in the reference; here it reads
 * (0, 0, 0, 0), like any out-of-range texture index.
 * ---------------------------------------------------------------------------------------- */
typedef struct { const orc_vertex *a, *b, *c; const orc_primitive *prim; float bx, by, bz, uvx, uvy; } orc_tri_fetch;
static inline uint8_t unorm8(float f);
static inline uint8_t srgb8(float c);

static orc_tri_fetch fetch_triangle(const orc_scene *s, uint32_t flat, float u, float v) {
    orc_tri_fetch f;
    const orc_tri *tr = &s->tris[flat];
    f.prim = &s->prims[tr->prim];                                                   /* gl_GeometryIndexEXT */
    uint32_t i0 = s->indices[f.prim->index_offset + 3 * tr->tri + 0];              /* gl_PrimitiveID */
    uint32_t i1 = s->indices[f.prim->index_offset + 3 * tr->tri + 1];
    uint32_t i2 = s->indices[f.prim->index_offset + 3 * tr->tri + 2];
    f.a = &s->vertices[f.prim->vertex_offset + i0];
    f.b = &s->vertices[f.prim->vertex_offset + i1];
    f.c = &s->vertices[f.prim->vertex_offset + i2];
    f.bx = 1.0f - u - v; f.by = u; f.bz = v;
    f.uvx = f.a->uv0[0] * f.bx + f.b->uv0[0] * f.by + f.c->uv0[0] * f.bz;
    f.uvy = f.a->uv0[1] * f.bx + f.b->uv0[1] * f.by + f.c->uv0[1] * f.bz;
    return f;
}

/* shadow_anyhit.rahit:8-27: 1 = ignoreIntersectionEXT */
static int alpha_ignored(const orc_scene *s, uint32_t flat, float u, float v) {
    orc_tri_fetch f = fetch_triangle(s, flat, u, v);                                 /* :9-20 */
    v4 albedo = sample_texture(s, f.prim->material.base_color_texture, f.uvx, f.uvy); /* :23 (unconditional) */
    return f.prim->material.alpha_mask == 1 && albedo.w < f.prim->material.alpha_cutoff;   /* :24-26 */
}

/* closesthit.rchit:10-58 (alpha == 0) / closesthit_test_alpha.rchit:10-51 (alpha == 1); returns the payload */
static v4 raytraced_closest_hit(const orc_scene *s, const orc_per_frame_data *pfd, const orc_hit *h, int alpha, int use_bvh,
                                uint64_t *rays) {
    orc_tri_fetch f = fetch_triangle(s, h->flat, h->u, h->v);                        /* :11-22 */
    const orc_vertex *a = f.a, *b = f.b, *c = f.c;
    float bx = f.bx, by = f.by, bz = f.bz;
    v3 normal = V3(a->normal[0] * bx + b->normal[0] * by + c->normal[0] * bz,       /* :23 object space, unnormalised */
                   a->normal[1] * bx + b->normal[1] * by + c->normal[1] * bz,
                   a->normal[2] * bx + b->normal[2] * by + c->normal[2] * bz);
    v3 opos = V3(a->pos[0] * bx + b->pos[0] * by + c->pos[0] * bz, a->pos[1] * bx + b->pos[1] * by + c->pos[1] * bz,
                 a->pos[2] * bx + b->pos[2] * by + c->pos[2] * bz);
    v3 position = mat4_mul_point(f.prim->transform, opos);                           /* :24 */
    v3 albedo;
    if (!alpha && f.prim->material.base_color_texture == -1)                        /* :26-32 */
        albedo = V3(f.prim->material.base_color[0], f.prim->material.base_color[1], f.prim->material.base_color[2]);
    else { v4 t = sample_texture(s, f.prim->material.base_color_texture, f.uvx, f.uvy); albedo = V3(t.x, t.y, t.z); }   /* alpha: :26 */
    v3 N = normal;                                                                   /* :34-41 */
    if (f.prim->material.normal_map >= 0) {
        v3 T = V3(a->tangent[0] * bx + b->tangent[0] * by + c->tangent[0] * bz, a->tangent[1] * bx + b->tangent[1] * by + c->tangent[1] * bz,
                  a->tangent[2] * bx + b->tangent[2] * by + c->tangent[2] * bz);
        float tw = a->tangent[3] * bx + b->tangent[3] * by + c->tangent[3] * bz;
        v4 tx = sample_texture(s, f.prim->material.normal_map, f.uvx, f.uvy);
        v3 tsn = normalize3(V3(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f));
        v3 bitangent = v3scale(cross3(tsn, T), tw);                                  /* sic: cross(tangent_space_normal, in_tangent.xyz) */
        v3 tangent = normalize3(v3sub(T, v3scale(normal, dot3(T, normal))));
        N = v3add(v3add(v3scale(tangent, tsn.x), v3scale(bitangent, tsn.y)), v3scale(normal, tsn.z));
    }
    v3 light_dir = v3neg(V3(pfd->directional_light.direction[0], pfd->directional_light.direction[1], pfd->directional_light.direction[2]));
    v3 lc = V3(pfd->directional_light.color[0], pfd->directional_light.color[1], pfd->directional_light.color[2]);
    v3 li = V3(pfd->directional_light.intensity[0], pfd->directional_light.intensity[1], pfd->directional_light.intensity[2]);
    v3 albedo_lighting = alpha ? v3scale(albedo, 0.2f) : v3scale(albedo, ORC_PI_INVERSE);   /* alpha :39 / :46 */
    /* shadow ray (:48-50 / alpha :41-43): payload starts true, shadow_miss.rmiss:7 clears it.  Without the any-hit
     * shader the ray terminates on the first hit; with it the walk runs to the end -- the boolean is the same */
    int shadowed = trace_filtered(s, position, light_dir, 0.1f, 10000.0f, 1, use_bvh, alpha).hit;
    ++*rays;
    v3 col = albedo_lighting;
    if (!shadowed) {                                                                 /* :52-54 / alpha :45-47 */
        float nl = fmaxf(dot3(N, light_dir), 0.0f);
        v3 lit = v3scale(albedo, nl);
        if (!alpha) lit = v3mul(lit, li);                                            /* the alpha variant drops light_intensity */
        lit = v3mul(lit, lc);
        col = v3add(albedo_lighting, lit);
    }
    v4 r = { col.x, col.y, col.z, 1.0f };
    return r;
}

void orc_raytraced(const orc_scene *s, const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                   int use_anyhit_shader, uint8_t *out_bgra8, uint64_t *rays_out, int use_bvh) {
    uint64_t rays = 0;
    int alpha = use_anyhit_shader != 0;
#pragma omp parallel for schedule(dynamic, 2) reduction(+ : rays)
    for (int64_t yy = (int64_t)row_begin; yy < (int64_t)row_end; ++yy) {
        uint32_t y = (uint32_t)yy;
        for (uint32_t x = 0; x < W; ++x) {
            float ux = (((float)x + 0.5f) / (float)W) * 2.0f - 1.0f;                 /* raygen.rgen:11-13 */
            float uy = (((float)y + 0.5f) / (float)H) * 2.0f - 1.0f;
            v4 origin = mat4_mul_v4(pfd->camera_view_inverse, (v4){ 0.0f, 0.0f, 0.0f, 1.0f });      /* :15 */
            v4 target = mat4_mul_v4(pfd->camera_proj_inverse, (v4){ ux, uy, 1.0f, 1.0f });          /* :16 */
            v3 tn = normalize3(V3(target.x, target.y, target.z));
            v4 direction = mat4_mul_v4(pfd->camera_view_inverse, (v4){ tn.x, tn.y, tn.z, 0.0f });   /* :17 */
            v4 payload = { 0.0f, 0.0f, 0.0f, 0.0f };                                                /* :19 */
            t_ray_pixel = y * W + x; t_ray_kind = ORC_RAY_KIND_PRIMARY;
            /* :20 gl_RayFlagsOpaqueEXT (alpha: gl_RayFlagsNoOpaqueEXT -> shadow_anyhit.rahit filters candidates), miss 0 */
            orc_hit h = trace_filtered(s, V3(origin.x, origin.y, origin.z), V3(direction.x, direction.y, direction.z), 0.1f, 10000.0f,
                                       0, use_bvh, alpha);
            ++rays;
            t_ray_kind = ORC_RAY_KIND_SHADOW;                                        /* closesthit.rchit's shadow ray */
            if (h.hit) payload = raytraced_closest_hit(s, pfd, &h, alpha, use_bvh, &rays);
            else payload = (v4){ 0.3f, 0.8f, 0.2f, 1.0f };                                          /* miss.rmiss:7 */
            t_ray_pixel = 0xffffffffu; t_ray_kind = ORC_RAY_KIND_OTHER;
            uint8_t *o = out_bgra8 + ((size_t)y * W + x) * 4;                        /* :22 imageStore to B8G8R8A8_UNORM */
            o[0] = unorm8(payload.z); o[1] = unorm8(payload.y); o[2] = unorm8(payload.x); o[3] = unorm8(payload.w);
        }
    }
    if (rays_out) *rays_out = rays;
}

/* raytraced_render_path/composition.vert:5-8 + composition.frag:11-13: the UNORM image sampled at the texel centre and
 * written to the B8G8R8A8_SRGB swapchain through the flipped presentation viewport (pipeline.cpp:175-178) */
void orc_raytraced_composition(uint32_t W, uint32_t H, const uint8_t *raytraced_bgra8, uint8_t *out_bgra8_srgb) {
    for (uint32_t j = 0; j < H; ++j) {
        uint32_t gy = H - 1 - j;
        for (uint32_t x = 0; x < W; ++x) {
            const uint8_t *p = raytraced_bgra8 + ((size_t)gy * W + x) * 4;
            uint8_t *o = out_bgra8_srgb + ((size_t)j * W + x) * 4;
            o[0] = srgb8(p[0] * (1.0f / 255.0f)); o[1] = srgb8(p[1] * (1.0f / 255.0f)); o[2] = srgb8(p[2] * (1.0f / 255.0f));
            o[3] = p[3];                                                             /* alpha is stored linearly */
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * stand-in G-buffer producer: primary rays, gbuf.frag encodings
 * ---------------------------------------------------------------------------------------- */
static void normal_matrix3(const float *m, float out[9]) {  /* inverseTranspose(mat3(transform)), hybrid_render_path.cpp:44 */
    double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    /* rows of M: (a b c), (d e f), (g h i); cofactor matrix / det == inverse transpose */
    double c00 = e * i - f * h, c01 = -(d * i - f * g), c02 = d * h - e * g;
    double c10 = -(b * i - c * h), c11 = a * i - c * g, c12 = -(a * h - b * g);
    double c20 = b * f - c * e, c21 = -(a * f - c * d), c22 = a * e - b * d;
    double det = a * c00 + b * c01 + c * c02;
    double id = det != 0.0 ? 1.0 / det : 0.0;
    /* out is column-major: out[col*3+row]; element (row r, col c) = cofactor(r,c)/det */
    out[0] = (float)(c00 * id); out[3] = (float)(c01 * id); out[6] = (float)(c02 * id);
    out[1] = (float)(c10 * id); out[4] = (float)(c11 * id); out[7] = (float)(c12 * id);
    out[2] = (float)(c20 * id); out[5] = (float)(c21 * id); out[8] = (float)(c22 * id);
}

#define ORC_GBUFFER_MAX_LAYERS 32   /* discarded surfaces a primary ray may step through */
static inline uint8_t unorm8(float f) {       /* UNORM store: clamp, round to nearest */
    if (!(f > 0.0f)) return 0;
    if (f >= 1.0f) return 255;
    return (uint8_t)(f * 255.0f + 0.5f);
}

void orc_gbuffer(const orc_scene *s, const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint16_t *normals_ids,
                 uint16_t *motion_mr, float *depth) {
    orc_gbuffer_albedo(s, pfd, W, H, normals_ids, motion_mr, depth, NULL);
}

void orc_gbuffer_albedo(const orc_scene *s, const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint16_t *normals_ids,
                        uint16_t *motion_mr, float *depth, uint8_t *albedo) {
    float *nm = (float *)malloc(sizeof(float) * 9 * (s->np ? s->np : 1));
    for (uint32_t p = 0; p < s->np; ++p) normal_matrix3(s->prims[p].transform, nm + 9 * p);
    float projview[16], prev_projview[16];
    orc_mat4_mul(pfd->camera_proj, pfd->camera_view, projview);
    orc_mat4_mul(pfd->camera_proj_prev_frame, pfd->camera_view_prev_frame, prev_projview);
    v3 cam = V3(pfd->camera_view_inverse[12], pfd->camera_view_inverse[13], pfd->camera_view_inverse[14]);
#pragma omp parallel for schedule(dynamic, 2)
    for (int64_t yy = 0; yy < (int64_t)H; ++yy) {
        int y = (int)yy;
        for (int x = 0; x < (int)W; ++x) {
            float u = ((float)x + 0.5f) / (float)W, v = ((float)y + 0.5f) / (float)H;
            v3 pnear = get_world_space_position(pfd, 1.0f, u, v);     /* reverse-Z: depth 1 == near plane */
            v3 dir = v3sub(pnear, cam);
            size_t px = (size_t)y * W + (size_t)x;
            /* Row f2: gbuf.frag:27-32 discards alpha-masked / fully transparent fragments, so the surface behind shows.
             * A primary-ray caster gets the same picture by stepping past a discarded hit (tmin = its t) and casting again. */
            orc_hit h;
            const orc_tri *tr = NULL;
            const orc_primitive *prim = NULL;
            const orc_vertex *a = NULL, *b = NULL, *c = NULL;
            float bx = 0, by = 0, bz = 0, uvx = 0, uvy = 0, tmin = 1.0f;
            v4 al = { 0, 0, 0, 0 };
            int visible = 0;
            t_ray_pixel = (uint32_t)px; t_ray_kind = ORC_RAY_KIND_PRIMARY;
            for (int layer = 0; layer < ORC_GBUFFER_MAX_LAYERS; ++layer) {
                h = trace(s, cam, dir, tmin, 3.0e38f, 0, 1);
                if (!h.hit) break;
                tr = &s->tris[h.flat];
                prim = &s->prims[tr->prim];
                uint32_t i0 = s->indices[prim->index_offset + 3 * tr->tri + 0];
                uint32_t i1 = s->indices[prim->index_offset + 3 * tr->tri + 1];
                uint32_t i2 = s->indices[prim->index_offset + 3 * tr->tri + 2];
                a = &s->vertices[prim->vertex_offset + i0];
                b = &s->vertices[prim->vertex_offset + i1];
                c = &s->vertices[prim->vertex_offset + i2];
                bx = 1.0f - h.u - h.v; by = h.u; bz = h.v;
                uvx = a->uv0[0] * bx + b->uv0[0] * by + c->uv0[0] * bz;
                uvy = a->uv0[1] * bx + b->uv0[1] * by + c->uv0[1] * bz;
                al = (v4){ prim->material.base_color[0], prim->material.base_color[1], prim->material.base_color[2], prim->material.base_color[3] };
                if (prim->material.base_color_texture != -1) al = sample_texture(s, prim->material.base_color_texture, uvx, uvy);   /* :19-26 */
                if ((prim->material.alpha_mask == 1 && al.w < prim->material.alpha_cutoff) || al.w == 0.0f) {                      /* :27-32 */
                    tmin = h.t;
                    continue;
                }
                visible = 1;
                break;
            }
            t_ray_pixel = 0xffffffffu; t_ray_kind = ORC_RAY_KIND_OTHER;
            if (!visible) {                                            /* clears: hybrid_render_path.cpp:16-19 */
                store_rgba16f(normals_ids, W, x, y, 0, 0, 0, 0);
                store_rgba16f(motion_mr, W, x, y, 0, 0, -1.0f, -1.0f);
                depth[px] = 0.0f;
                if (albedo) memset(albedo + px * 4, 0, 4);
                continue;
            }
            v3 P = v3add(cam, v3scale(dir, h.t));
            v4 clip = mat4_mul_v4(projview, (v4){ P.x, P.y, P.z, 1.0f });
            depth[px] = clip.z / clip.w;
            v3 n = V3(a->normal[0] * bx + b->normal[0] * by + c->normal[0] * bz,
                      a->normal[1] * bx + b->normal[1] * by + c->normal[1] * bz,
                      a->normal[2] * bx + b->normal[2] * by + c->normal[2] * bz);
            v3 N = n;
            if (prim->material.normal_map >= 0) {                       /* gbuf.frag:35-41 */
                v4 tx = sample_texture(s, prim->material.normal_map, uvx, uvy);
                v3 tsn = normalize3(V3(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f));
                v3 T = V3(a->tangent[0] * bx + b->tangent[0] * by + c->tangent[0] * bz,
                          a->tangent[1] * bx + b->tangent[1] * by + c->tangent[1] * bz,
                          a->tangent[2] * bx + b->tangent[2] * by + c->tangent[2] * bz);
                float tw = a->tangent[3] * bx + b->tangent[3] * by + c->tangent[3] * bz;
                v3 bitangent = v3scale(cross3(tsn, T), tw);              /* sic: cross(tangent_space_normal, in_tangent.xyz) */
                v3 tangent = normalize3(v3sub(T, v3scale(n, dot3(T, n))));
                N = v3add(v3add(v3scale(tangent, tsn.x), v3scale(bitangent, tsn.y)), v3scale(n, tsn.z));
            }
            const float *M = nm + 9 * tr->prim;
            v3 wn = V3((M[0] * N.x + M[3] * N.y) + M[6] * N.z, (M[1] * N.x + M[4] * N.y) + M[7] * N.z,
                       (M[2] * N.x + M[5] * N.y) + M[8] * N.z);
            wn = normalize3(wn);                                        /* gbuf.frag:43 */
            store_rgba16f(normals_ids, W, x, y, wn.x, wn.y, wn.z, (float)tr->prim);
            /* gbuf.frag:46-47: current = gl_FragCoord.xy * display_size_inverse, prev = reprojected ndc*0.5+0.5 */
            float cx = ((float)x + 0.5f) * pfd->display_size_inverse[0];
            float cy = ((float)y + 0.5f) * pfd->display_size_inverse[1];
            v4 rp = mat4_mul_v4(prev_projview, (v4){ P.x, P.y, P.z, 1.0f });
            float px_ = (rp.x / rp.w) * 0.5f + 0.5f, py_ = (rp.y / rp.w) * 0.5f + 0.5f;
            float metallic = prim->material.metallic_factor, roughness = prim->material.roughness_factor;
            if (prim->material.metallic_roughness_texture != -1) {    /* gbuf.frag:50-56 */
                v4 mr = sample_texture(s, prim->material.metallic_roughness_texture, uvx, uvy);
                metallic *= mr.y; roughness *= mr.z;
            }
            if (albedo) {                                              /* gbuf.frag:33 */
                uint8_t *o = albedo + px * 4;                          /* B8G8R8A8 */
                o[0] = unorm8(al.z); o[1] = unorm8(al.y); o[2] = unorm8(al.x); o[3] = unorm8(al.w);
            }
            store_rgba16f(motion_mr, W, x, y, cx - px_, cy - py_, metallic, roughness);   /* gbuf.frag:58 */
        }
    }
    free(nm);
}

/* ------------------------------------------------------------------------------------------
 * composition.frag:60-161 (next row f3)
 * ---------------------------------------------------------------------------------------- */
static inline uint8_t srgb8(float c) {          /* B8G8R8A8_SRGB store: NaN -> 0, clamp, encode, round */
    if (!(c > 0.0f)) return 0;
    if (c >= 1.0f) return 255;
    double e = c <= 0.0031308 ? 12.92 * c : 1.055 * pow((double)c, 1.0 / 2.4) - 0.055;
    return (uint8_t)(e * 255.0 + 0.5);
}

/* the default sampler (decision x), defined with the screen-space shaders below */
typedef v4 (*orc_texel_fn)(const void *img, uint32_t W, int x, int y);
static v4 texel_d32f(const void *img, uint32_t W, int x, int y);
static v4 sample_linear_repeat(orc_texel_fn fetch, const void *img, uint32_t W, uint32_t H, float u, float v);

/* Stand-in for the "Shadow Map Pass" (hybrid_render_path.cpp:58-99, depth_prepass.vert:16-19): the reference rasterises the scene
 * with directional_light.projview into a 4096 x 4096 D32 image, cleared to 0, depth test GREATER_OR_EQUAL (reverse Z: 1 on the near
 * plane).  Decision (xiv): texel (i, j) holds the depth of the closest hit of the orthographic ray through its centre -- from
 * the near plane (NDC z = 1) to the far plane (z = 0), depth = 1 - t with t the ray parameter in (0, 1) -- or the clear value. */
void orc_shadow_map(const orc_scene *s, const orc_per_frame_data *pfd, uint32_t size, uint32_t row_begin, uint32_t row_end, float *shadow_map,
                    int use_bvh) {
    float inv[16];
    orc_mat4_inverse(pfd->directional_light.projview, inv);
#pragma omp parallel for schedule(dynamic, 8)
    for (int64_t jj = (int64_t)row_begin; jj < (int64_t)row_end; ++jj) {
        int j = (int)jj;
        for (int i = 0; i < (int)size; ++i) {
            float nx = (((float)i + 0.5f) / (float)size) * 2.0f - 1.0f, ny = (((float)j + 0.5f) / (float)size) * 2.0f - 1.0f;
            v4 a = mat4_mul_v4(inv, (v4){ nx, ny, 1.0f, 1.0f }), b = mat4_mul_v4(inv, (v4){ nx, ny, 0.0f, 1.0f });
            v3 o = V3(a.x / a.w, a.y / a.w, a.z / a.w), f = V3(b.x / b.w, b.y / b.w, b.z / b.w);
            orc_hit h = trace(s, o, v3sub(f, o), 0.0f, 1.0f, 0, use_bvh);
            shadow_map[(size_t)j * size + i] = h.hit ? 1.0f - h.t : 0.0f;
        }
    }
}

/* orc_composition with the lighting before the B8G8R8A8_SRGB store as a second output (tests/composition_cases.py judges a device texel by it):
 * `lighting`, when not NULL, receives r, g, b of composition.frag:158 per texel, in the presented orientation of `out`. */
void orc_composition_lit(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, int shadow_mode, int ao_mode, int reflection_mode,
                         const uint8_t *albedo_img, const uint16_t *normals_ids, const uint16_t *motion_mr, const float *depth,
                         const uint16_t *shadow_ao, int shadow_ao_channels, const uint16_t *reflections, const uint16_t *ssao,
                         const float *shadow_map, uint32_t shadow_map_size, uint8_t *out, float *lighting_out) {
    /* composition.frag:82 `SHADOW_BIAS_MATRIX * pfd.directional_light.projview * vec4(P, 1)`: the matrix product first */
    static const float bias[16] = { 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.5f, 0.5f, 0.0f, 1.0f };   /* common.glsl:6-11 */
    float bias_projview[16];
    orc_mat4_mul(bias, pfd->directional_light.projview, bias_projview);
#pragma omp parallel for schedule(static)
    for (int64_t jj = 0; jj < (int64_t)H; ++jj) {
        int j = (int)jj;
        int gy = (int)H - 1 - j;                                  /* flipped presentation viewport, pipeline.cpp:175-178 */
        for (int x = 0; x < (int)W; ++x) {
            float u = ((float)x + 0.5f) / (float)W, v = ((float)gy + 0.5f) / (float)H;       /* composition.vert:6 at the texel centre */
            const uint8_t *ap = albedo_img + ((size_t)gy * W + x) * 4;
            v3 albedo = V3(ap[2] * (1.0f / 255.0f), ap[1] * (1.0f / 255.0f), ap[0] * (1.0f / 255.0f));   /* :61 */
            float d = depth[(size_t)gy * W + x];                                               /* :62 */
            v3 P = get_world_space_position(pfd, d, u, v);                                     /* :63 */
            v4 nid = load_rgba16f(normals_ids, W, x, gy);                                      /* :64 */
            v3 N = V3(nid.x, nid.y, nid.z);
            v4 mm = load_rgba16f(motion_mr, W, x, gy);                                         /* :65 .zw */
            float rs = 1.0f, ra = 1.0f;                                                        /* :67-70 */
            if (shadow_mode == 0 || ao_mode == 0) {
                v4 t = shadow_ao_channels == 4 ? load_rgba16f(shadow_ao, W, x, gy) : load_rg16f(shadow_ao, W, x, gy);
                rs = t.x; ra = t.y;
            }
            v3 cam = V3(pfd->camera_view_inverse[12], pfd->camera_view_inverse[13], pfd->camera_view_inverse[14]);
            v3 Vv = normalize3(v3sub(cam, P));                                                 /* :72-75 */
            v3 L = v3neg(V3(pfd->directional_light.direction[0], pfd->directional_light.direction[1], pfd->directional_light.direction[2]));
            v3 Hh = normalize3(v3add(L, Vv));
            float shadow = shadow_mode == 0 ? rs : 1.0f;                                       /* :77-80 */
            if (shadow_mode == 1) {                                                            /* :81-107: 16-tap PCF on the shadow map */
                v4 pl = mat4_mul_v4(bias_projview, (v4){ P.x, P.y, P.z, 1.0f });
                float sx = pl.x / pl.w, sy = pl.y / pl.w, sz = pl.z / pl.w;
                const float scale = 1.0f / 4096.0f;
                float lit = 0.0f;
                for (int i = 0; i < 16; ++i) {
                    float ox = ((float)(i >> 2) - 1.5f) * scale, oy = ((float)(i & 3) - 1.5f) * scale;    /* offsets[i], :88-93 */
                    float ds = sample_linear_repeat(texel_d32f, shadow_map, shadow_map_size, shadow_map_size, sx + ox, sy + oy).x;
                    lit += (sz < ds - 1e-4f) ? 0.0f : 1.0f;
                }
                shadow = lit / 16.0f;
            }
            float ao = ao_mode == 0 ? ra : 1.0f;                                               /* :114-121 */
            if (ao_mode == 1) ao = load_rgba16f(ssao, W, x, gy).x;                             /* :117-119: texture() at a texel centre */
            float metallic = fminf(fmaxf(mm.z, 0.0f), 1.0f);                                   /* :123-125 */
            float roughness = fminf(fmaxf(mm.w, 0.04f), 1.0f);
            v3 li = V3(pfd->directional_light.intensity[0], pfd->directional_light.intensity[1], pfd->directional_light.intensity[2]);
            v3 lc = V3(pfd->directional_light.color[0], pfd->directional_light.color[1], pfd->directional_light.color[2]);
            v3 f0 = V3(0.04f * (1.0f - metallic) + albedo.x * metallic, 0.04f * (1.0f - metallic) + albedo.y * metallic,
                       0.04f * (1.0f - metallic) + albedo.z * metallic);                       /* :131-132 */
            v3 F = fresnel_schlick(f0, Hh, Vv);
            float ndl = fmaxf(dot3(N, L), 0.0f);                                               /* :135 */
            v3 ambient = v3scale(albedo, ao * ORC_PI_INVERSE);                                 /* :137 */
            v3 diff = v3scale(v3mul(v3mul(v3scale(diffuse_brdf(metallic, albedo, F), ndl), li), lc), shadow);   /* :138 */
            v3 spec = v3scale(v3mul(v3mul(v3scale(specular_brdf(roughness, F, Vv, L, N, Hh), ndl), li), lc), shadow);   /* :139 */
            if (reflection_mode == 0 || reflection_mode == 1) {                                /* :139-156, ray traced or screen space */
                v4 r = load_rgba16f(reflections, W, x, gy);
                v3 refl = v3scale(V3(r.x, r.y, r.z), shadow);
                if (metallic == 1.0f) spec = refl;
                else spec = V3(mixf(spec.x, refl.x, roughness), mixf(spec.y, refl.y, roughness), mixf(spec.z, refl.z, roughness));
            }
            v3 lighting = v3add(v3add(ambient, diff), spec);                                   /* :160-162 */
            uint8_t *o = out + ((size_t)j * W + x) * 4;
            o[0] = srgb8(lighting.z); o[1] = srgb8(lighting.y); o[2] = srgb8(lighting.x); o[3] = 255;
            if (lighting_out) {
                float *lo = lighting_out + ((size_t)j * W + x) * 3;
                lo[0] = lighting.x; lo[1] = lighting.y; lo[2] = lighting.z;
            }
        }
    }
}

void orc_composition(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, int shadow_mode, int ao_mode, int reflection_mode,
                     const uint8_t *albedo_img, const uint16_t *normals_ids, const uint16_t *motion_mr, const float *depth,
                     const uint16_t *shadow_ao, int shadow_ao_channels, const uint16_t *reflections, const uint16_t *ssao,
                     const float *shadow_map, uint32_t shadow_map_size, uint8_t *out) {
    orc_composition_lit(pfd, W, H, shadow_mode, ao_mode, reflection_mode, albedo_img, normals_ids, motion_mr, depth, shadow_ao, shadow_ao_channels,
                        reflections, ssao, shadow_map, shadow_map_size, out, NULL);
}

/* ------------------------------------------------------------------------------------------
 * next row f4 (second half): the screen-space alternatives of the hybrid render path
 *   data/shaders/hybrid_render_path/ssao.comp:14-53, ssao_blur.comp:11-26, ssr.comp:16-137
 * Decisions (the reference leaves them to the Vulkan implementation):
 *  (x)   texture() on a transient image goes through the default sampler (LINEAR mag / min, REPEAT,
 *        resource_manager.cpp:58-69) at LOD 0: unnormalised coordinate u * W - 0.5, floor, the four texels wrapped,
 *        weights in full fp32 (hardware uses 8 fractional bits), blended x first then y;
 *  (xi)  the shaders declare their output images r16f, the images are R16G16B16A16_SFLOAT (hybrid_render_path.cpp:149,
 *        176,219): all four components of the stored vec4 land in the texel;
 *  (xii) min / max / clamp drop a NaN operand (IEEE minNum / maxNum, what the author's hardware does; GLSL leaves it
 *        undefined) -- sky samples produce inf and NaN view-space positions, which then contribute 0;
 *  (xiii) float -> int of the coordinates saturates and maps NaN to 0 (f2i above).
 * ---------------------------------------------------------------------------------------- */
static inline int wrap_repeat(int i, int n) { int m = i % n; return m < 0 ? m + n : m; }

static v4 texel_rgba16f(const void *img, uint32_t W, int x, int y) { return load_rgba16f((const uint16_t *)img, W, x, y); }
static v4 texel_d32f(const void *img, uint32_t W, int x, int y) {
    v4 r = { ((const float *)img)[(size_t)y * W + x], 0.0f, 0.0f, 1.0f };
    return r;
}
static v4 texel_bgra8(const void *img, uint32_t W, int x, int y) {      /* B8G8R8A8_UNORM sampled as (r, g, b, a) */
    const uint8_t *p = (const uint8_t *)img + ((size_t)y * W + x) * 4;
    v4 r = { p[2] * (1.0f / 255.0f), p[1] * (1.0f / 255.0f), p[0] * (1.0f / 255.0f), p[3] * (1.0f / 255.0f) };
    return r;
}
/* decision (x) */
static v4 sample_linear_repeat(orc_texel_fn fetch, const void *img, uint32_t W, uint32_t H, float u, float v) {
    float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
    float x0f = floorf(fx), y0f = floorf(fy);
    float ax = fx - x0f, ay = fy - y0f;
    int x0 = wrap_repeat(f2i(x0f), (int)W), y0 = wrap_repeat(f2i(y0f), (int)H);
    int x1 = x0 + 1 == (int)W ? 0 : x0 + 1, y1 = y0 + 1 == (int)H ? 0 : y0 + 1;
    v4 t00 = fetch(img, W, x0, y0), t10 = fetch(img, W, x1, y0), t01 = fetch(img, W, x0, y1), t11 = fetch(img, W, x1, y1);
    float bx = 1.0f - ax, by = 1.0f - ay;
    v4 r;
    r.x = (t00.x * bx + t10.x * ax) * by + (t01.x * bx + t11.x * ax) * ay;
    r.y = (t00.y * bx + t10.y * ax) * by + (t01.y * bx + t11.y * ax) * ay;
    r.z = (t00.z * bx + t10.z * ax) * by + (t01.z * bx + t11.z * ax) * ay;
    r.w = (t00.w * bx + t10.w * ax) * by + (t01.w * bx + t11.w * ax) * ay;
    return r;
}
void orc_sample_linear_repeat(int kind, const void *img, uint32_t W, uint32_t H, float u, float v, float out[4]) {
    v4 r = sample_linear_repeat(kind == 0 ? texel_rgba16f : kind == 1 ? texel_d32f : texel_bgra8, img, W, H, u, v);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

/* glsl_common.h:111-115 */
static v3 get_view_space_position(const orc_per_frame_data *pfd, float depth, float u, float v) {
    v4 ndc = { u * 2.0f - 1.0f, v * 2.0f - 1.0f, depth, 1.0f };
    v4 r = mat4_mul_v4(pfd->camera_proj_inverse, ndc);
    return V3(r.x / r.w, r.y / r.w, r.z / r.w);
}

/* ssao.comp:14-53.  radius: SSAOPushConstants.radius (see the note on orc_ssao in the header). */
void orc_ssao(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
              const uint16_t *normals_ids, const float *depth, float radius, uint16_t *ssao_raw) {
    const float *cv = pfd->camera_view;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t yy = (int64_t)row_begin; yy < (int64_t)row_end; ++yy) {
        int y = (int)yy;
        for (int x = 0; x < (int)W; ++x) {
            float cu = (float)x * pfd->display_size_inverse[0], cvv = (float)y * pfd->display_size_inverse[1];      /* :15 */
            float current_depth = sample_linear_repeat(texel_d32f, depth, W, H, cu, cvv).x;                         /* :16 */
            if (current_depth == 0.0f) { store_rgba16f(ssao_raw, W, x, y, 0.0f, 0.0f, 0.0f, 0.0f); continue; }      /* :17-24 */
            v3 P = get_view_space_position(pfd, current_depth, cu, cvv);                                            /* :25 */
            v4 n4 = sample_linear_repeat(texel_rgba16f, normals_ids, W, H, cu, cvv);
            v3 N = V3((cv[0] * n4.x + cv[4] * n4.y) + cv[8] * n4.z, (cv[1] * n4.x + cv[5] * n4.y) + cv[9] * n4.z,
                      (cv[2] * n4.x + cv[6] * n4.y) + cv[10] * n4.z);                                               /* :26 mat3(view) * n */
            float perspective_radius = radius / P.z;                                                                /* :28-29 */
            const float beta = 1e-4f;                                                                               /* :30-31 */
            uint32_t rng = orc_seed_thread(((uint32_t)y * (uint32_t)pfd->display_size[1] + (uint32_t)x) * pfd->frame_index);   /* :32 */
            float sum = 0.0f;
            for (int i = 0; i < 16; ++i) {                                                                          /* :33-45 */
                float ang = (orc_random01(&rng) * 2.0f) * ORC_PI;
                float dist = orc_random01(&rng) * perspective_radius;
                float sn, cs;
                orc_sincos(ang, &sn, &cs);
                float su = cu + cs * dist, sv = cvv + sn * dist;
                v3 Q = get_view_space_position(pfd, sample_linear_repeat(texel_d32f, depth, W, H, su, sv).x, su, sv);
                v3 V = v3sub(Q, P);
                sum += fmaxf(dot3(V, N) - beta, 0.0f) / (dot3(V, V) + 1e-4f);
            }
            float ao = fmaxf(1.0f - ((2.0f * 1.0f) / 16.0f) * sum, 0.0f);                                           /* :47 */
            store_rgba16f(ssao_raw, W, x, y, ao, ao, ao, ao);                                                       /* :49-53, decision (xi) */
        }
    }
}

/* ssao_blur.comp:11-26: 13x13 box over the texels inside the display, always divided by 169 */
void orc_ssao_blur(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                   const uint16_t *ssao_raw, uint16_t *ssao_blurred) {
#pragma omp parallel for schedule(static)
    for (int64_t yy = (int64_t)row_begin; yy < (int64_t)row_end; ++yy) {
        int cy = (int)yy;
        for (int cx = 0; cx < (int)W; ++cx) {
            float ao = 0.0f;
            for (int y = -6; y <= 6; ++y)
                for (int x = -6; x <= 6; ++x) {
                    int sx = cx + x, sy = cy + y;
                    if (sx < 0 || (float)sx >= pfd->display_size[0] || sy < 0 || (float)sy >= pfd->display_size[1]) continue;
                    if ((uint32_t)sx >= W || (uint32_t)sy >= H) continue;                     /* imageLoad outside the image returns 0 */
                    ao += load_rgba16f(ssao_raw, W, sx, sy).x;
                }
            float r = ao / (13.0f * 13.0f);
            store_rgba16f(ssao_blurred, W, cx, cy, r, r, r, r);
        }
    }
}

static inline float distance3(v3 a, v3 b) { v3 d = v3sub(a, b); return sqrtf(dot3(d, d)); }
static inline float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

/* ssr.comp:16-137.  albedo: B8G8R8A8_UNORM; output RGBA16F = (lighting, 1) or 0 */
void orc_ssr(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
             const uint8_t *albedo_bgra8, const uint16_t *normals_ids, const uint16_t *motion_mr, const float *depth,
             float ray_distance, float step_size, float thickness, int32_t bsearch_steps, uint16_t *ssr_out) {
    float projview[16];
    orc_mat4_mul(pfd->camera_proj, pfd->camera_view, projview);                               /* :23 proj * view, then * vec4 */
    const v3 cam = V3(pfd->camera_view_inverse[12], pfd->camera_view_inverse[13], pfd->camera_view_inverse[14]);
    const int n_steps = f2i(ray_distance / step_size);                                        /* :83 */
#pragma omp parallel for schedule(dynamic, 2)
    for (int64_t yy = (int64_t)row_begin; yy < (int64_t)row_end; ++yy) {
        int y = (int)yy;
        for (int x = 0; x < (int)W; ++x) {
            float cu = (float)x * pfd->display_size_inverse[0], cvv = (float)y * pfd->display_size_inverse[1];      /* :68 */
            float fragment_depth = sample_linear_repeat(texel_d32f, depth, W, H, cu, cvv).x;
            v3 P = get_world_space_position(pfd, fragment_depth, cu, cvv);                                          /* :72 */
            v4 n4 = sample_linear_repeat(texel_rgba16f, normals_ids, W, H, cu, cvv);
            v3 N = V3(n4.x, n4.y, n4.z);
            v3 I = normalize3(v3sub(P, cam));                                                                       /* :74 */
            float ni2 = 2.0f * dot3(N, I);
            v3 rdir = normalize3(v3sub(I, v3scale(N, ni2)));                                                        /* :75 */
            int found = 0;
            float prev_step = 0.0f, final_step = 0.0f;
            float fu = 0.0f, fv = 0.0f;
            for (int i = 0; i < n_steps; ++i) {                                                                     /* :83-101 */
                float offset = step_size * (float)i;
                v3 rp = v3add(P, v3scale(rdir, offset));
                float d_ray = distance3(cam, rp);
                v4 clip = mat4_mul_v4(projview, (v4){ rp.x, rp.y, rp.z, 1.0f });                                    /* :22-26 */
                float su = (clip.x / clip.w) * 0.5f + 0.5f, sv = (clip.y / clip.w) * 0.5f + 0.5f;
                v3 sp = get_world_space_position(pfd, sample_linear_repeat(texel_d32f, depth, W, H, su, sv).x, su, sv);
                float delta = d_ray - distance3(cam, sp);
                if (delta > 0.3f && delta < thickness) { final_step = offset; found = 1; break; }
                prev_step = offset;
            }
            if (!found) { store_rgba16f(ssr_out, W, x, y, 0.0f, 0.0f, 0.0f, 0.0f); continue; }                      /* :62-66, 103-105 */
            float mid_step = (prev_step + final_step) * 0.5f;                                                       /* :108 */
            for (int i = 0; i < bsearch_steps; ++i) {                                                               /* :110-128 */
                v3 rp = v3add(P, v3scale(rdir, mid_step));
                float d_ray = distance3(cam, rp);
                v4 clip = mat4_mul_v4(projview, (v4){ rp.x, rp.y, rp.z, 1.0f });
                fu = (clip.x / clip.w) * 0.5f + 0.5f; fv = (clip.y / clip.w) * 0.5f + 0.5f;
                v3 sp = get_world_space_position(pfd, sample_linear_repeat(texel_d32f, depth, W, H, fu, fv).x, fu, fv);
                float delta = d_ray - distance3(cam, sp);
                if (delta > 0.3f && delta < thickness) {
                    mid_step = (prev_step + mid_step) * 0.5f;
                } else {
                    float tmp = mid_step;
                    mid_step = mid_step + (mid_step - prev_step);
                    prev_step = tmp;
                }
            }
            /* compute_lighting(final_uv), :28-59 */
            v4 a4 = sample_linear_repeat(texel_bgra8, albedo_bgra8, W, H, fu, fv);
            v3 albedo = V3(a4.x, a4.y, a4.z);
            v3 position = get_world_space_position(pfd, sample_linear_repeat(texel_d32f, depth, W, H, fu, fv).x, fu, fv);
            v4 mm = sample_linear_repeat(texel_rgba16f, motion_mr, W, H, fu, fv);
            v3 Vv = normalize3(v3sub(cam, position));
            v3 L = v3neg(V3(pfd->directional_light.direction[0], pfd->directional_light.direction[1], pfd->directional_light.direction[2]));
            v4 ln = sample_linear_repeat(texel_rgba16f, normals_ids, W, H, fu, fv);
            v3 Nl = V3(ln.x, ln.y, ln.z);
            v3 Hh = normalize3(v3add(L, Vv));
            float metallic = clampf(mm.z, 0.0f, 1.0f);
            float roughness = clampf(mm.w, 0.04f, 1.0f);
            float ambient_factor = ORC_PI_INVERSE * 0.2f;
            v3 li = V3(pfd->directional_light.intensity[0], pfd->directional_light.intensity[1], pfd->directional_light.intensity[2]);
            v3 lc = V3(pfd->directional_light.color[0], pfd->directional_light.color[1], pfd->directional_light.color[2]);
            v3 f0 = V3(mixf(0.04f, albedo.x, metallic), mixf(0.04f, albedo.y, metallic), mixf(0.04f, albedo.z, metallic));
            v3 F = fresnel_schlick(f0, Hh, Vv);
            v3 ambient = v3scale(albedo, ambient_factor);
            v3 diff = diffuse_brdf(metallic, albedo, F);
            v3 spec = specular_brdf(roughness, F, Vv, L, Nl, Hh);
            float ndl = fmaxf(dot3(Nl, L), 0.0f);
            v3 lit = v3add(ambient, v3mul(v3mul(v3scale(v3add(diff, spec), ndl), li), lc));
            store_rgba16f(ssr_out, W, x, y, lit.x, lit.y, lit.z, 1.0f);                                             /* :131-135 */
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * svgf.comp
 * ---------------------------------------------------------------------------------------- */
/* svgf.comp:16-39 */
static int is_valid_reprojection(const orc_per_frame_data *pfd, const uint16_t *prev_normals, uint32_t W, int px, int py,
                                 int current_object_id, v3 current_normal) {
    if (px < 0 || py < 0 || (float)px >= pfd->display_size[0] || (float)py >= pfd->display_size[1]) return 0;
    v4 pn = load_rgba16f(prev_normals, W, px, py);
    int prev_id = f2i(pn.w);
    if (current_object_id != prev_id) return 0;
    if (dot3(current_normal, V3(pn.x, pn.y, pn.z)) < ORC_COS_PI_4) return 0;
    return 1;
}

/* svgf.comp:41-145 */
void orc_svgf_temporal(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, const uint16_t *normals_ids,
                       const uint16_t *motion_mr, const uint16_t *raytraced, const uint16_t *prev_normals_ids,
                       const uint16_t *history, const uint16_t *moments_in, uint16_t *integrated_out, uint16_t *moments_out) {
#pragma omp parallel for schedule(static)
    for (int64_t yy = 0; yy < (int64_t)H; ++yy) {
        int cy = (int)yy;
        for (int cx = 0; cx < (int)W; ++cx) {
            v4 nid = load_rgba16f(normals_ids, W, cx, cy);                                 /* :43-45 */
            v3 current_normal = V3(nid.x, nid.y, nid.z);
            int current_object_id = f2i(nid.w);
            v4 mv = load_rgba16f(motion_mr, W, cx, cy);                                    /* :46 */
            v4 cur = load_rg16f(raytraced, W, cx, cy);                                     /* :47-49 */
            float current_shadow = cur.x, current_ao = cur.y;

            float pcx = ((float)cx - mv.x * pfd->display_size[0]) + 0.5f;                  /* :52 */
            float pcy = ((float)cy - mv.y * pfd->display_size[1]) + 0.5f;
            float x = pcx - floorf(pcx);                                                    /* :53-54 fract */
            float y = pcy - floorf(pcy);
            int ax = f2i(pcx), ay = f2i(pcy);                                               /* :55 truncation */
            float bw[4] = { (1.0f - x) * (1.0f - y), x * (1.0f - y), (1.0f - x) * y, x * y };  /* :57 */
            static const int off[4][2] = { { 0, 0 }, { 1, 0 }, { 0, 1 }, { 1, 1 } };

            float prev_shadow = 0.0f, prev_ao = 0.0f, sum = 0.0f;
            float psm0 = 0.0f, psm1 = 0.0f, pam0 = 0.0f, pam1 = 0.0f;
            for (int i = 0; i < 4; ++i) {                                                   /* :65-77 */
                int sx = ax + off[i][0], sy = ay + off[i][1];
                if (is_valid_reprojection(pfd, prev_normals_ids, W, sx, sy, current_object_id, current_normal)) {
                    v4 hs = load_rgba16f(history, W, sx, sy);
                    prev_shadow += bw[i] * hs.x;
                    prev_ao += bw[i] * hs.y;
                    v4 m = load_rg16f(moments_in, W, sx, sy);
                    psm0 += bw[i] * m.x; psm1 += bw[i] * m.y;
                    pam0 += bw[i] * m.z; pam1 += bw[i] * m.w;
                    sum += bw[i];
                }
            }
            int valid = sum > 1e-6f;                                                        /* :78 */
            if (!valid) {                                                                   /* :81-97 (accumulators not reset) */
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        int sx = ax + dx, sy = ay + dy;
                        if (is_valid_reprojection(pfd, prev_normals_ids, W, sx, sy, current_object_id, current_normal)) {
                            v4 hs = load_rgba16f(history, W, sx, sy);
                            v4 m = load_rg16f(moments_in, W, sx, sy);
                            prev_shadow += hs.x; prev_ao += hs.y;
                            psm0 += m.x; psm1 += m.y; pam0 += m.z; pam1 += m.w;
                            sum += 1.0f;
                        }
                    }
                valid = sum > 1e-6f;
            }
            float sm0 = current_shadow, sm1 = current_shadow * current_shadow;              /* :99-102 */
            float am0 = current_ao, am1 = current_ao * current_ao;
            if (valid) {                                                                    /* :106-126 */
                const float alpha = 0.2f, moments_alpha = 0.2f;
                prev_shadow /= sum; psm0 /= sum; psm1 /= sum;
                prev_ao /= sum; pam0 /= sum; pam1 /= sum;
                sm0 = mixf(psm0, sm0, moments_alpha); sm1 = mixf(psm1, sm1, moments_alpha);
                am0 = mixf(pam0, am0, moments_alpha); am1 = mixf(pam1, am1, moments_alpha);
                float sv = fmaxf(0.0f, sm1 - sm0 * sm0);
                float av = fmaxf(0.0f, am1 - am0 * am0);
                store_rgba16f(integrated_out, W, cx, cy, mixf(prev_shadow, current_shadow, alpha),
                              mixf(prev_ao, current_ao, alpha), sv, av);
            } else {                                                                        /* :127-135 */
                float sv = fmaxf(0.0f, sm1 - sm0 * sm0);
                float av = fmaxf(0.0f, am1 - am0 * am0);
                store_rgba16f(integrated_out, W, cx, cy, current_shadow, current_ao, sv, av);
            }
            store_rg16f(moments_out, W, cx, cy, sm0, sm1);                                  /* :138-144 into an RG16F image */
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * svgf_atrous_filter.comp
 * ---------------------------------------------------------------------------------------- */
static inline float pow128(float x) {   /* decision (v) */
    if (!(x > 0.0f)) return 0.0f;
    x *= x; x *= x; x *= x; x *= x; x *= x; x *= x; x *= x;
    return x;
}
/* :48-51 */
static inline float edge_stopping_luminance(float variance_p, float lp, float lq) {
    float e = fabsf(lp - lq) / (4.0f * sqrtf(variance_p) + 1e-6f);
    return expf(-e);
}

void orc_svgf_atrous(const orc_per_frame_data *pfd, uint32_t W, uint32_t H, const uint16_t *normals_ids,
                     const uint16_t *in, uint16_t *out, int32_t step) {
    static const float gauss[9] = { 1.0f / 16, 1.0f / 8, 1.0f / 16, 1.0f / 8, 1.0f / 4, 1.0f / 8, 1.0f / 16, 1.0f / 8, 1.0f / 16 };
    static const float k5[25] = { 1.0f / 256, 1.0f / 64, 3.0f / 128, 1.0f / 64, 1.0f / 256,
                                  1.0f / 64,  1.0f / 16, 3.0f / 32,  1.0f / 16, 1.0f / 64,
                                  3.0f / 128, 3.0f / 32, 9.0f / 64,  3.0f / 32, 3.0f / 128,
                                  1.0f / 64,  1.0f / 16, 3.0f / 32,  1.0f / 16, 1.0f / 64,
                                  1.0f / 256, 1.0f / 64, 3.0f / 128, 1.0f / 64, 1.0f / 256 };
    const float dsx = pfd->display_size[0], dsy = pfd->display_size[1];
#pragma omp parallel for schedule(static)
    for (int64_t yy = 0; yy < (int64_t)H; ++yy) {
        int cy = (int)yy;
        for (int cx = 0; cx < (int)W; ++cx) {
            v4 np = load_rgba16f(normals_ids, W, cx, cy);                                   /* :55-57 */
            v3 normal_p = V3(np.x, np.y, np.z);
            int id_p = f2i(np.w);
            v4 p = load_rgba16f(in, W, cx, cy);                                             /* :59 */
            float var_s = 0.0f, var_a = 0.0f;                                               /* :17-38 gauss_3x3_filter */
            for (int y = -1; y <= 1; ++y)
                for (int x = -1; x <= 1; ++x) {
                    int sx = cx + x, sy = cy + y;
                    if (sx < 0 || (float)sx >= dsx || sy < 0 || (float)sy >= dsy) continue;
                    float w = gauss[3 * (y + 1) + (x + 1)];
                    v4 q = load_rgba16f(in, W, sx, sy);
                    var_s += w * q.z;
                    var_a += w * q.w;
                }
            float sw_s = 1.0f, sw_a = 1.0f;                                                 /* :70-71 */
            float s0 = p.x, s1 = p.y, s2 = p.z, s3 = p.w;
            for (int y = -2; y <= 2; ++y)
                for (int x = -2; x <= 2; ++x) {                                             /* :72-94 */
                    int sx = cx + x * step, sy = cy + y * step;
                    if (sx < 0 || (float)sx >= dsx || sy < 0 || (float)sy >= dsy || (x == 0 && y == 0)) continue;
                    v4 q = load_rgba16f(in, W, sx, sy);
                    float kernel = k5[5 * (y + 2) + (x + 2)];
                    v4 nq = load_rgba16f(normals_ids, W, sx, sy);
                    float wn = fmaxf(0.0f, pow128(dot3(normal_p, V3(nq.x, nq.y, nq.z))));  /* :44-46 */
                    float wid = (id_p == f2i(nq.w)) ? 1.0f : 0.0f;                          /* :40-42 */
                    float w = kernel * wn * wid;
                    float wx = w * edge_stopping_luminance(var_s, p.x, q.x);
                    float wy = w * edge_stopping_luminance(var_a, p.y, q.y);
                    sw_s += wx; sw_a += wy;
                    s0 += wx * q.x; s1 += wy * q.y; s2 += (wx * wx) * q.z; s3 += (wy * wy) * q.w;
                }
            store_rgba16f(out, W, cx, cy, s0 / sw_s, s1 / sw_a, s2 / (sw_s * sw_s), s3 / (sw_a * sw_a));  /* :97-101 */
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * host schedule: hybrid_render_path.cpp:245-331
 * ---------------------------------------------------------------------------------------- */
struct orc_svgf_state {
    uint32_t W, H;
    uint16_t *img[5];          /* 0,1 integrated ping-pong; 2 prev normals; 3 history; 4 moments (RG16F) */
    uint16_t *moments_snapshot;
    int x, y;                  /* svgf_push_constants.integrated_shadow_and_ao.{x,y} */
};

orc_svgf_state *orc_svgf_create(uint32_t W, uint32_t H) {
    orc_svgf_state *st = (orc_svgf_state *)calloc(1, sizeof *st);
    st->W = W; st->H = H;
    size_t px = (size_t)W * H;
    for (int i = 0; i < 4; ++i) st->img[i] = (uint16_t *)calloc(px * 4, 2);     /* :247-258 (decision viii: zeroed) */
    st->img[4] = (uint16_t *)calloc(px * 2, 2);                                   /* :259-261 R16G16 */
    st->moments_snapshot = (uint16_t *)calloc(px * 2, 2);
    st->x = 0; st->y = 1;
    return st;
}
void orc_svgf_destroy(orc_svgf_state *st) {
    if (!st) return;
    for (int i = 0; i < 5; ++i) free(st->img[i]);
    free(st->moments_snapshot);
    free(st);
}
const uint16_t *orc_svgf_image(const orc_svgf_state *st, int which) {
    if (which == 0) return st->img[st->x];
    if (which == 1) return st->img[st->y];
    return st->img[which];
}

void orc_svgf_frame(orc_svgf_state *st, const orc_per_frame_data *pfd, const uint16_t *normals_ids, const uint16_t *motion_mr,
                    const uint16_t *raytraced, uint16_t *denoised_out) {
    const uint32_t W = st->W, H = st->H;
    const size_t px = (size_t)W * H;
    /* :291-297 svgf.comp (decision ii: moments read from a snapshot) */
    memcpy(st->moments_snapshot, st->img[4], px * 2 * 2);
    orc_svgf_temporal(pfd, W, H, normals_ids, motion_mr, raytraced, st->img[2], st->img[3], st->moments_snapshot,
                      st->img[st->x], st->img[4]);
    for (int i = 0; i < 5; ++i) {                                                 /* :299-319 */
        orc_svgf_atrous(pfd, W, H, normals_ids, st->img[st->x], st->img[st->y], 1 << i);
        if (i == 0) memcpy(st->img[3], st->img[st->y], px * 4 * 2);               /* :310-315 */
        int t = st->x; st->x = st->y; st->y = t;                                  /* :318 */
    }
    memcpy(st->img[2], normals_ids, px * 4 * 2);                                  /* :321 */
    memcpy(denoised_out, st->img[st->y], px * 4 * 2);                             /* :322-325 */
    { int t = st->x; st->x = st->y; st->y = t; }                                  /* :328 */
}

int orc_struct_sizes(uint32_t out[8]) {
    out[0] = sizeof(orc_vertex); out[1] = sizeof(orc_material); out[2] = sizeof(orc_primitive);
    out[3] = sizeof(orc_directional_light); out[4] = sizeof(orc_per_frame_data); out[5] = sizeof(orc_trace_params);
    out[6] = 0; out[7] = 0;
    return 6;
}

int orc_max_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}
