// Film grain for the waifu2x video / image routes on gfx950: counter-based normal noise, apply_rgb_noise, the temporal blend
// of the noise buffer, the fused per-frame video step, and frame_to_tensor with a quarter turn folded into its gather.
//
// Reference: nunif/utils/rgb_noise.py rgb_noise_like :5-18 (randn_like; level 2: 0.5 * n1 + 0.5 * nearest_up(randn(H//2, W//2))),
// apply_rgb_noise :21-39; waifu2x/ui_utils.py process_video frame_callback :154-177 (rot90, the noise buffer
// `buf = buf * (1 - speed) + noise * speed`, or `buf = noise` after a shape change :169-171, apply, VU.to_frame);
// nunif/utils/video.py from_tensor :236-245 ((x * max).round().to(uint)), to_tensor :218-223.
//
// The random stream is Philox-4x32-10 (Salmon et al., SC'11) keyed by the 64-bit seed, counter = (x >> 2, plane * H + y,
// frame counter, component): a value depends on its coordinates only, never on launch shape, tile order or stream.  Values are
// NOT torch's for any seed (torch's Philox offsets follow its own launch geometry); the distribution is what the tests pin.
//
// Everything here is a streaming kernel.  The fused step moves 39 B per output pixel at 8 bit (12 B frame read, 12 B + 12 B noise
// buffer read + write, 3 B HWC store; 42 B at 16 bit) against the reference's ~25 fp32 passes.  A lane owns 4 consecutive pixels:
// planar accesses are 16 B, the HWC store 12 B (8 bit) or 3 x 8 B (16 bit).  The noise buffer stays fp32: an fp16 buffer would
// put 2^-11 * |noise| * strength ~ 1e-4 into the linear-domain result, three orders above the reference's own fp32 error.
// -ffp-contract=off: the fused kernel and the separate launches evaluate the same expressions with the same roundings.
#include "common.h"

namespace nunif {

struct GrainKey { uint32_t k0, k1, c2, c3; };          // seed lo / hi, frame counter lo, (frame counter hi << 1) | component

struct ApplyParams {                                   // apply_rgb_noise's scalars, rounded to fp32 the way torch rounds them
    float gamma, inv_gamma, strength, lds, one_minus_lds;
    int light_decay;
};

struct BlendParams { float speed, one_minus_speed; int first; };

__device__ __forceinline__ f32x4 philox_normal4(GrainKey key, uint32_t group, uint32_t row, uint32_t component) {
    uint32_t c0 = group, c1 = row, c2 = key.c2, c3 = key.c3 | component, k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    // Box-Muller on 24-bit uniforms: u in (0, 1] for the radius (|z| <= 5.77), v in [0, 1) turns for the angle
    const float s = 1.0f / 16777216.0f;
    const float m2ln2 = -1.3862943611198906f;                          // -2 ln u = -2 ln 2 * log2 u
    const float ra = sqrtf(m2ln2 * __log2f((float)((c0 >> 8) + 1u) * s)), ta = 6.2831853071795865f * ((float)(c1 >> 8) * s);
    const float rb = sqrtf(m2ln2 * __log2f((float)((c2 >> 8) + 1u) * s)), tb = 6.2831853071795865f * ((float)(c3 >> 8) * s);
    return (f32x4){ra * __cosf(ta), ra * __sinf(ta), rb * __cosf(tb), rb * __sinf(tb)};
}

__device__ __forceinline__ float pick4(f32x4 v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// torch's `nearest` source index (upsample_nearest: min(floorf(dst * scale), in - 1) with scale = (float)in / out)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    const int s = (int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

struct NoiseGeom { int H, W, H2, W2; float sy, sx; };

__host__ __device__ inline NoiseGeom noise_geom(int H, int W) {
    NoiseGeom g;
    g.H = H; g.W = W; g.H2 = H / 2; g.W2 = W / 2;
    g.sy = g.H2 > 0 ? (float)g.H2 / (float)H : 0.f;
    g.sx = g.W2 > 0 ? (float)g.W2 / (float)W : 0.f;
    return g;
}

// the four noise values of pixels x0 .. x0+3 (x0 % 4 == 0) of row y of plane p; component 0: rgb_noise_like(level), 1: n1 alone,
// 2: the upsampled n2 alone.  Lanes beyond W are computed and ignored by the caller.
__device__ __forceinline__ f32x4 noise4(GrainKey key, NoiseGeom g, int level, int component, int plane, int y, int x0) {
    f32x4 n1 = {0.f, 0.f, 0.f, 0.f}, n2 = {0.f, 0.f, 0.f, 0.f};
    if (component != 2) n1 = philox_normal4(key, (uint32_t)x0 >> 2, (uint32_t)plane * (uint32_t)g.H + (uint32_t)y, 0u);
    if (component == 1 || (component == 0 && level == 1)) return n1;
    const uint32_t row2 = (uint32_t)plane * (uint32_t)g.H2 + (uint32_t)nearest_src(y, g.sy, g.H2);
    const int c0 = nearest_src(x0, g.sx, g.W2);
    const f32x4 a = philox_normal4(key, (uint32_t)c0 >> 2, row2, 1u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cx = nearest_src(x0 + j, g.sx, g.W2);
        n2[j] = (cx >> 2) == (c0 >> 2) ? pick4(a, cx & 3) : pick4(philox_normal4(key, (uint32_t)cx >> 2, row2, 1u), cx & 3);
    }
    if (component == 2) return n2;
    return n1 * 0.5f + n2 * 0.5f;                                      // noise.mul_(0.5).add_(noise2, alpha=0.5)
}

__device__ __forceinline__ float blend1(float buf, float noise, BlendParams b) {
    return b.first ? noise : buf * b.one_minus_speed + noise * b.speed;          // ui_utils.py:169-174
}

// x ** g for x in [0, 1] as exp2(g * log2 x) on the hardware's 1-ulp v_log_f32 / v_exp_f32: exact at 0 and 1; for normal x the
// relative error is about (1 + |g log2 x|) * 2^-23, i.e. below 2e-7 of a value that is itself below 2^-|g log2 x| — in the linear
// domain the tests measure, the same order as fp32 rounding (bound and measurement in tests/test_gpu_grain.py).  Both
// instructions flush fp32 denormals: an input or a result below 1.2e-38 becomes exactly 0 where powf would return a tiny positive
// value (1e-38 ** (1 / 2.2) ~ 5e-18) — nothing after quantisation or in the linear domain.  A negative or NaN input gives NaN
// here as in the reference's pow; the clamps around it (fmaxf / fminf drop a NaN operand) then turn it into 0, where the reference
// carries the NaN through to the frame.  The library powf costs ~250 instructions a call; three of them per value would make
// this kernel ALU-bound at several times its memory time.
__device__ __forceinline__ float pow01(float x, float g) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(g * __builtin_amdgcn_logf(x));
#else
    return 0.f;                    // host pass of the single-source compile only parses this
#endif
}

__device__ __forceinline__ float apply1(float rgb, float noise, ApplyParams a) {
    float out = pow01(rgb, a.gamma);                                    // rgb ** gamma
    const float correlated = noise * out;
    float weight = a.strength;
    if (a.light_decay) weight = pow01((1.0f - out) * a.lds + a.one_minus_lds, a.gamma) * a.strength;
    out = out + correlated * weight;
    return pow01(fminf(fmaxf(out, 0.f), 1.f), a.inv_gamma);             // clamp_(0, 1).pow_(1 / gamma)
}

template <typename T>
__device__ __forceinline__ T quantise(float v, float maxv) {           // stereo_to_frame_kernel's clamp + (x * max).round()
    return (T)rintf(fminf(fmaxf(v, 0.f), 1.f) * maxv);
}

// ---- generator ---------------------------------------------------------------------------------------------------------
// out [planes, H, W] (component 0..2) or the n2 grid itself [planes, H / 2, W / 2] (component 3; H, W are then the grid's own)
__global__ void __launch_bounds__(256)
rgb_noise_kernel(float *__restrict__ out, int planes, NoiseGeom g, int level, int component, GrainKey key, int vec) {
    const int W4 = (g.W + 3) >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)planes * g.H * W4) return;
    const int x0 = (int)(i % W4) << 2;
    const long t = i / W4;
    const int y = (int)(t % g.H), p = (int)(t / g.H);
    f32x4 v;
    if (component == 3) v = philox_normal4(key, (uint32_t)x0 >> 2, (uint32_t)p * (uint32_t)g.H + (uint32_t)y, 1u);
    else v = noise4(key, g, level, component, p, y, x0);
    float *dst = out + ((long)p * g.H + y) * g.W + x0;
    if (vec) *(f32x4 *)dst = v;
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (x0 + j < g.W) dst[j] = v[j];
    }
}

// ---- blend / apply as launches of their own ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
grain_blend_kernel(float *__restrict__ buf, const float *__restrict__ noise, long n, BlendParams b, int vec) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const f32x4 nz = *(const f32x4 *)(noise + i);
        f32x4 o = nz;
        if (!b.first) {
            const f32x4 old = *(const f32x4 *)(buf + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = blend1(old[j], nz[j], b);
        }
        *(f32x4 *)(buf + i) = o;
    } else {
        for (long j = i; j < n && j < i + 4; ++j) buf[j] = blend1(b.first ? 0.f : buf[j], noise[j], b);
    }
}

__global__ void __launch_bounds__(256)
apply_rgb_noise_kernel(const float *__restrict__ rgb, const float *__restrict__ noise, float *__restrict__ out, long n,
                       ApplyParams a, int vec) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const f32x4 x = *(const f32x4 *)(rgb + i), nz = *(const f32x4 *)(noise + i);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = apply1(x[j], nz[j], a);
        *(f32x4 *)(out + i) = o;
    } else {
        for (long j = i; j < n && j < i + 4; ++j) out[j] = apply1(rgb[j], noise[j], a);
    }
}

// ---- the fused video step ----------------------------------------------------------------------------------------------
struct __attribute__((aligned(4))) Px4x8 { uint32_t w[3]; };            // 4 HWC pixels, 8 bit: 12 B
struct __attribute__((aligned(8))) Px4x16 { u32x2 w[3]; };             // 4 HWC pixels, 16 bit: 24 B

// rgb, buf: [3, H, W] fp32; frame: HWC.  VEC: W % 4 == 0 and all pointers aligned (the host checks) — a lane owns 4 pixels.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
grain_video_step_kernel(const float *__restrict__ rgb, float *__restrict__ buf, T *__restrict__ frame, NoiseGeom g, int level,
                        GrainKey key, BlendParams b, ApplyParams a, float maxv) {
    const int W4 = (g.W + 3) >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.H * W4) return;
    const int x0 = (int)(i % W4) << 2, y = (int)(i / W4);
    const long hw = (long)g.H * g.W, p0 = (long)y * g.W + x0;
    T q[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f32x4 nz = noise4(key, g, level, 0, c, y, x0);
        const float *src = rgb + c * hw + p0;
        float *nb = buf + c * hw + p0;
        if (VEC) {
            const f32x4 x = *(const f32x4 *)src;
            f32x4 o = nz;
            if (!b.first) {
                const f32x4 old = *(const f32x4 *)nb;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = blend1(old[j], nz[j], b);
            }
            *(f32x4 *)nb = o;
#pragma unroll
            for (int j = 0; j < 4; ++j) q[c][j] = quantise<T>(apply1(x[j], o[j], a), maxv);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x0 + j < g.W) {
                    const float o = blend1(b.first ? 0.f : nb[j], nz[j], b);
                    nb[j] = o;
                    q[c][j] = quantise<T>(apply1(src[j], o, a), maxv);
                }
            }
        }
    }
    T *dst = frame + p0 * 3;
    if (VEC) {
        if (sizeof(T) == 1) {
            Px4x8 o;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const int idx = k * 4 + e; w |= (uint32_t)q[idx % 3][idx / 3] << (8 * e); }
                o.w[k] = w;
            }
            *(Px4x8 *)dst = o;
        } else {
            Px4x16 o;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int i0 = 2 * k, i1 = 2 * k + 1;
                o.w[k >> 1][k & 1] = (uint32_t)q[i0 % 3][i0 / 3] | ((uint32_t)q[i1 % 3][i1 / 3] << 16);
            }
            *(Px4x16 *)dst = o;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j < g.W) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[j * 3 + c] = q[c][j];
            }
        }
    }
}

// ---- frame_to_tensor with a quarter turn -------------------------------------------------------------------------------
// in HWC [H, W, 3] -> out [3, W, H] = rot90(to_tensor(in), turns, (-2, -1)).  turns 1: r[i][j] = x[j][W-1-i]; turns 3: r[i][j] =
// x[H-1-j][i] (the index map of image_ops.hip view_src).  32 x 32 tiles through the LDS: the frame (often pinned host memory read
// over PCIe) is read along its rows, the planes are written along theirs.
template <typename T>
__global__ void __launch_bounds__(256)
frame_to_tensor_rot_kernel(const T *__restrict__ in, float *__restrict__ out, int H, int W, int turns, float maxv) {
    __shared__ float tile[3][32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ly = ty + 8 * r, sy = y0 + ly, sx = x0 + tx;
        if (sy < H && sx < W) {
            const T *px = in + ((long)sy * W + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) tile[c][ly][tx] = (float)px[c] / maxv;      // x / iinfo.max (true division, fp32)
        }
    }
    __syncthreads();
    const long hw = (long)H * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lx = ty + 8 * r, ly = tx, sy = y0 + ly, sx = x0 + lx;             // lanes run along the source column
        if (sy < H && sx < W) {
            const long o = turns == 1 ? (long)(W - 1 - sx) * H + sy : (long)sx * H + (H - 1 - sy);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * hw + o] = tile[c][ly][lx];
        }
    }
}

static GrainKey make_key(uint64_t seed, uint64_t counter) {
    GrainKey k;
    k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32);
    k.c2 = (uint32_t)counter; k.c3 = (uint32_t)(counter >> 32) << 1;
    return k;
}

static bool make_apply(double strength, double gamma, int light_decay, double lds, ApplyParams *a) {
    if (!(gamma > 0.0) || !(lds >= 0.0 && lds <= 1.0)) return false;
    a->gamma = (float)gamma; a->inv_gamma = (float)(1.0 / gamma); a->strength = (float)strength;
    a->lds = (float)lds; a->one_minus_lds = (float)(1.0 - lds); a->light_decay = light_decay ? 1 : 0;
    return true;
}

static BlendParams make_blend(double speed, int first) {
    BlendParams b;
    b.speed = (float)speed; b.one_minus_speed = (float)(1.0 - speed); b.first = first ? 1 : 0;
    return b;
}

static inline bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_rgb_noise(float *out, int32_t planes, int32_t H, int32_t W, int32_t level, int32_t component,
                                   uint64_t seed, uint64_t counter, void *stream) {
    NUNIF_REQUIRE(out && planes > 0 && H > 0 && W > 0 && (level == 1 || level == 2) && component >= 0 && component <= 3,
                  "rgb_noise: bad argument");
    NUNIF_REQUIRE(counter < (1ull << 63), "rgb_noise: counter must be below 2^63");
    const bool needs_grid = component >= 2 || (component == 0 && level == 2);
    NUNIF_REQUIRE(!needs_grid || (H >= 2 && W >= 2), "rgb_noise: level 2 needs H >= 2 and W >= 2");
    NUNIF_REQUIRE((long)planes * H < (1L << 32), "rgb_noise: planes * H must be below 2^32");
    hipStream_t s = (hipStream_t)stream;
    NoiseGeom g = noise_geom(H, W);
    if (component == 3) { g.H = H / 2; g.W = W / 2; }                  // the launch covers the grid itself
    const long lanes = (long)planes * g.H * ((g.W + 3) / 4);
    ProfScope ps("rgb_noise_kernel", s, 0.0, (double)planes * g.H * g.W * 4.0);
    const int vec = (g.W % 4 == 0) && aligned_to(out, 16);
    rgb_noise_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(out, planes, g, level, component, make_key(seed, counter), vec);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_apply_rgb_noise(const float *rgb, const float *noise, float *out, int64_t n, double strength,
                                         double gamma, int32_t light_decay, double light_decay_strength, void *stream) {
    ApplyParams a;
    NUNIF_REQUIRE(rgb && noise && out && n > 0, "apply_rgb_noise: bad argument");
    NUNIF_REQUIRE(make_apply(strength, gamma, light_decay, light_decay_strength, &a),
                  "apply_rgb_noise: gamma must be positive and light_decay_strength in [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("apply_rgb_noise_kernel", s, 0.0, (double)n * 12.0);
    const int vec = aligned_to(rgb, 16) && aligned_to(noise, 16) && aligned_to(out, 16);
    const long lanes = (n + 3) / 4;
    apply_rgb_noise_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(rgb, noise, out, n, a, vec);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_grain_blend(float *buf, const float *noise, int64_t n, double speed, int32_t first, void *stream) {
    NUNIF_REQUIRE(buf && noise && n > 0, "grain_blend: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("grain_blend_kernel", s, 0.0, (double)n * (first ? 8.0 : 12.0));
    const int vec = aligned_to(buf, 16) && aligned_to(noise, 16);
    const long lanes = (n + 3) / 4;
    grain_blend_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(buf, noise, n, make_blend(speed, first), vec);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_grain_video_step(const float *rgb, float *noise_buffer, void *frame, int32_t H, int32_t W,
                                          int32_t bits, int32_t level, uint64_t seed, uint64_t counter, double speed,
                                          int32_t first, double strength, double gamma, int32_t light_decay,
                                          double light_decay_strength, void *stream) {
    ApplyParams a;
    NUNIF_REQUIRE(rgb && noise_buffer && frame && H > 0 && W > 0 && (bits == 8 || bits == 16) && (level == 1 || level == 2),
                  "grain_video_step: bad argument");
    NUNIF_REQUIRE(level == 1 || (H >= 2 && W >= 2), "grain_video_step: level 2 needs H >= 2 and W >= 2");
    NUNIF_REQUIRE(counter < (1ull << 63), "grain_video_step: counter must be below 2^63");
    NUNIF_REQUIRE(make_apply(strength, gamma, light_decay, light_decay_strength, &a),
                  "grain_video_step: gamma must be positive and light_decay_strength in [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    const NoiseGeom g = noise_geom(H, W);
    const GrainKey key = make_key(seed, counter);
    const BlendParams b = make_blend(speed, first);
    const long lanes = (long)H * ((W + 3) / 4);
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    ProfScope ps("grain_video_step_kernel", s, 0.0, (double)H * W * ((first ? 24.0 : 36.0) + 3.0 * bits / 8));
    const bool vec = (W % 4 == 0) && aligned_to(rgb, 16) && aligned_to(noise_buffer, 16) && aligned_to(frame, 8);
    if (bits == 8) {
        if (vec) grain_video_step_kernel<uint8_t, true><<<blocks, 256, 0, s>>>(rgb, noise_buffer, (uint8_t *)frame, g, level, key, b, a, 255.0f);
        else grain_video_step_kernel<uint8_t, false><<<blocks, 256, 0, s>>>(rgb, noise_buffer, (uint8_t *)frame, g, level, key, b, a, 255.0f);
    } else {
        if (vec) grain_video_step_kernel<uint16_t, true><<<blocks, 256, 0, s>>>(rgb, noise_buffer, (uint16_t *)frame, g, level, key, b, a, 65535.0f);
        else grain_video_step_kernel<uint16_t, false><<<blocks, 256, 0, s>>>(rgb, noise_buffer, (uint16_t *)frame, g, level, key, b, a, 65535.0f);
    }
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_frame_to_tensor_rot(const void *frame, float *chw, int32_t H, int32_t W, int32_t bits, int32_t turns,
                                             void *stream) {
    NUNIF_REQUIRE(frame && chw && H > 0 && W > 0 && (bits == 8 || bits == 16) && (turns == 1 || turns == 3),
                  "frame_to_tensor_rot: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("frame_to_tensor_rot_kernel", s, 0.0, (double)H * W * (3.0 * bits / 8 + 12.0));
    const dim3 grid((unsigned)cdiv(W, 32), (unsigned)cdiv(H, 32));
    if (bits == 8) frame_to_tensor_rot_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t *)frame, chw, H, W, turns, 255.0f);
    else frame_to_tensor_rot_kernel<uint16_t><<<grid, 256, 0, s>>>((const uint16_t *)frame, chw, H, W, turns, 65535.0f);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
