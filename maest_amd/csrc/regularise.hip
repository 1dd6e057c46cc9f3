// Training-time regularisers of the MAEST blocks: element dropout (pos_drop, Attention.proj_drop, Mlp.drop) and stochastic depth
// (DropPath) -- reference: models/maest.py:200-207, 354-377, 404-419, 532-546, 800; models/helpers/vit_helpers.py drop_path.
//
// Masks are never stored: every kernel recomputes them from a counter-based generator (Philox4x32-10) whose counter is made of the
// element's COORDINATES (clip, token, column), the site and the step -- the definition is in include/maest_hip.h.  One Philox call
// yields four 32-bit words = the keep decisions of the four consecutive columns a lane holds as a float4 / 4 x 16-bit group, so the
// generator rides in the streaming kernels that move those 16 bytes anyway.  (seed, step) are read from a small DEVICE snapshot
// written by maest_rng_advance on the forward's stream: a captured training graph draws fresh masks at every replay, and the
// backward of a forward reads the same snapshot the forward did.
//
// HBM-bound row kernels in the style of norm.hip: one wave64 per 768-wide row, 3 x 16-byte loads per lane.
#include "common.h"

namespace maest {

constexpr int RG_COLS = 768;
constexpr int RG_VEC = 3;  // float4 per lane

struct philox4 { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): counter c0..c3, key k0, k1
__host__ __device__ __forceinline__ philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    philox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// what a kernel needs to draw masks: the (seed, step) snapshot and the two sites of a residual branch (site < 0: that part is off)
struct DropArgs {
    const uint32_t* snap;  // {seed lo, seed hi, step, 0}
    int n_tok;             // N: tokens of a full clip (the coordinate system of the element counter)
    int rows_per_clip;     // rows of a clip in THIS buffer: token t = row % rows_per_clip
    int site_e; uint32_t thr_e; float scale_e;
    int site_p; uint32_t thr_p; float scale_p;
};

// multipliers of the four columns [c, c + 4) (c % 4 == 0) of (clip b, token t) at an element site of width C: scale where kept, else 0
__device__ __forceinline__ void elem_mult4(const uint32_t* snap, int n_tok, int b, int t, int C, int c, int site, uint32_t thr, float scale,
                                           float (&m)[4]) {
    const uint64_t e = (((uint64_t)b * (uint64_t)n_tok + (uint64_t)t) * (uint64_t)C + (uint64_t)c) >> 2;
    const philox4 r = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)site, snap[2], snap[0], snap[1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = r.w[j] >= thr ? scale : 0.0f;
}
// multiplier of clip b at a drop-path site
__device__ __forceinline__ float path_mult(const uint32_t* snap, int b, int site, uint32_t thr, float scale) {
    const philox4 r = philox4x32_10((uint32_t)b >> 2, 0u, (uint32_t)site, snap[2], snap[0], snap[1]);
    return r.w[b & 3] >= thr ? scale : 0.0f;
}

__device__ __forceinline__ void rg_load4(const void* p, int dtype, int64_t off, float (&o)[4]) {
    if (dtype == MAEST_BF16) {
        const chunk8 t = *reinterpret_cast<const chunk8*>(reinterpret_cast<const bf16_t*>(p) + off);
        o[0] = lo16f(t[0]); o[1] = hi16f(t[0]); o[2] = lo16f(t[1]); o[3] = hi16f(t[1]);
    } else {
        const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + off);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    }
}
__device__ __forceinline__ void rg_store4(void* p, int dtype, int64_t off, float a, float b, float c, float d) {
    if (dtype == MAEST_BF16) {
        chunk8 o;
        o[0] = pack_bf2(a, b);
        o[1] = pack_bf2(c, d);
        *reinterpret_cast<chunk8*>(reinterpret_cast<bf16_t*>(p) + off) = o;
    } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + off) = make_float4(a, b, c, d);
    }
}

// snapshot <- state; state.step += 1.  One lane; ordered on the stream like every other launch of the forward.
__global__ void rng_advance_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ snapshot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const uint32_t lo = state[0], hi = state[1], step = state[2];
        snapshot[0] = lo; snapshot[1] = hi; snapshot[2] = step; snapshot[3] = 0u;
        state[2] = step + 1u;
    }
}

// In-place element dropout of x (and of `aux`, same shape: the saved gelu' beside gelu at the Mlp site): one 16-byte vector per thread
// and trip -- 4 fp32 columns (one Philox call) or 8 16-bit columns (two).
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(T* __restrict__ x, T* __restrict__ aux, int64_t n_vec, int C, DropArgs a) {
    constexpr int PER = elem_traits<T>::kPerChunk;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * 256) {
        const int64_t off = v * PER;
        const int64_t row = off / C;
        const int c = (int)(off - row * C);
        const int b = (int)(row / a.rows_per_clip), t = (int)(row - (int64_t)b * a.rows_per_clip);
        float m[PER];
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            float mq[4];
            elem_mult4(a.snap, a.n_tok, b, t, C, c + 4 * q, a.site_e, a.thr_e, a.scale_e, mq);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[4 * q + j] = mq[j];
        }
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            T* p = w == 0 ? x : aux;
            if (p == nullptr) continue;
            chunk16 d = *reinterpret_cast<const chunk16*>(p + off);
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = f2u(u2f(d[j]) * m[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = pack_bf2(lo16f(d[j]) * m[2 * j], hi16f(d[j]) * m[2 * j + 1]);
            }
            *reinterpret_cast<chunk16*>(p + off) = d;
        }
    }
}

// x_out = x + (delta * keep_e * scale_e) * keep_p * scale_p, and (LN) y = LayerNorm(x_out): maest_add_layernorm_fwd with the branch
// multiplier.  !LN: the add alone (last block, head-token tail, truncated forward).  CAST: dst = cast(src * multiplier), no add -- the
// gradient entering a regularised branch.
template <bool LN, bool CAST>
__global__ __launch_bounds__(256) void drop_row_kernel(const float* __restrict__ x, const void* __restrict__ delta, int delta_dtype,
                                                       float* __restrict__ x_out, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, void* __restrict__ y, int y_dtype,
                                                       float* __restrict__ mean, float* __restrict__ rstd, int rows, float eps, DropArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;  // wave-uniform
    const int b = row / a.rows_per_clip, t = row - b * a.rows_per_clip;
    const float mp = a.site_p >= 0 ? path_mult(a.snap, b, a.site_p, a.thr_p, a.scale_p) : 1.0f;
    float v[4 * RG_VEC];
#pragma unroll
    for (int i = 0; i < RG_VEC; ++i) {
        const int c = i * 256 + lane * 4;
        const int64_t off = (int64_t)row * RG_COLS + c;
        float d[4], m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (CAST) rg_load4(x, MAEST_F32, off, d);
        else rg_load4(delta, delta_dtype, off, d);
        if (a.site_e >= 0) elem_mult4(a.snap, a.n_tok, b, t, RG_COLS, c, a.site_e, a.thr_e, a.scale_e, m);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (a.site_e >= 0) d[e] = d[e] * m[e];
            if (a.site_p >= 0) d[e] = d[e] * mp;
        }
        if (CAST) {
            rg_store4(y, y_dtype, off, d[0], d[1], d[2], d[3]);
        } else {
            const float4 xv = *reinterpret_cast<const float4*>(x + off);
            v[4 * i] = d[0] + xv.x; v[4 * i + 1] = d[1] + xv.y; v[4 * i + 2] = d[2] + xv.z; v[4 * i + 3] = d[3] + xv.w;
            *reinterpret_cast<float4*>(x_out + off) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        }
    }
    if constexpr (LN) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 4 * RG_VEC; ++i) s += v[i];
        const float mu = wave_sum(s) * (1.0f / RG_COLS);
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < 4 * RG_VEC; ++i) { const float dd = v[i] - mu; q += dd * dd; }
        const float var = wave_sum(q) * (1.0f / RG_COLS);
        const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
        for (int i = 0; i < RG_VEC; ++i) {
            const int c = i * 256 + lane * 4;
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 bt = *reinterpret_cast<const float4*>(beta + c);
            rg_store4(y, y_dtype, (int64_t)row * RG_COLS + c, (v[4 * i] - mu) * rs * g.x + bt.x, (v[4 * i + 1] - mu) * rs * g.y + bt.y,
                      (v[4 * i + 2] - mu) * rs * g.z + bt.z, (v[4 * i + 3] - mu) * rs * g.w + bt.w);
        }
        if (lane == 0) {
            if (mean) mean[row] = mu;
            if (rstd) rstd[row] = rs;
        }
    }
}

static bool drop_args_ok(const char* who, int B, int N, int rpc, int cols, int site_e, int site_p, const void* snapshot) {
    if (snapshot == nullptr) { set_error("%s: null pointer", who); return false; }
    if (cols != RG_COLS) { set_error("%s: cols must be 768, got %d", who, cols); return false; }
    if (B <= 0 || N <= 0 || rpc <= 0 || rpc > N || (int64_t)B * rpc > 0x7fffffffll) {
        set_error("%s: bad shape B=%d N=%d rows per clip=%d", who, B, N, rpc);
        return false;
    }
    if (site_e < 0 && site_p < 0) { set_error("%s: no site: the element part and the path part are both off", who); return false; }
    return true;
}

}  // namespace maest

using namespace maest;

extern "C" int maest_rng_advance(uint32_t* state, uint32_t* snapshot, void* stream) {
    MAEST_REQUIRE(state && snapshot, "maest_rng_advance: null pointer");
    MAEST_REQUIRE(state != snapshot, "maest_rng_advance: the snapshot must not alias the state");
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, snapshot);
    return check_launch("maest_rng_advance");
}

extern "C" int maest_dropout(void* x, void* aux, int dtype, int B, int N, int n_rows_per_clip, int C, uint32_t thr, float scale,
                             int site, const uint32_t* snapshot, void* stream) {
    MAEST_REQUIRE(x && snapshot, "maest_dropout: null pointer");
    MAEST_REQUIRE(dtype == MAEST_F32 || dtype == MAEST_BF16, "maest_dropout: bad dtype");
    MAEST_REQUIRE(B > 0 && N > 0 && n_rows_per_clip > 0 && n_rows_per_clip <= N, "maest_dropout: bad shape B=%d N=%d rows per clip=%d", B, N,
                  n_rows_per_clip);
    MAEST_REQUIRE(C > 0 && C % 8 == 0, "maest_dropout: C must be a positive multiple of 8, got %d", C);
    MAEST_REQUIRE(site >= 0, "maest_dropout: site=%d", site);
    MAEST_REQUIRE(x != aux, "maest_dropout: aux must not alias x");
    const int per = dtype == MAEST_F32 ? 4 : 8;
    const int64_t n_vec = (int64_t)B * n_rows_per_clip * C / per;
    const int64_t want = (n_vec + 255) / 256;
    const int blocks = (int)(want < 8192 ? want : 8192);
    DropArgs a{snapshot, N, n_rows_per_clip, site, thr, scale, -1, 0u, 1.0f};
    if (dtype == MAEST_F32)
        hipLaunchKernelGGL(dropout_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)x, (float*)aux, n_vec, C, a);
    else
        hipLaunchKernelGGL(dropout_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, (bf16_t*)aux, n_vec, C, a);
    return check_launch("maest_dropout");
}

extern "C" int maest_drop_add_layernorm_fwd(const float* x, const void* delta, int delta_dtype, float* x_out, const float* gamma,
                                            const float* beta, void* y, int y_dtype, float* mean, float* rstd, int B, int N,
                                            int n_rows_per_clip, int cols, float eps, int site_e, uint32_t thr_e, float scale_e,
                                            int site_p, uint32_t thr_p, float scale_p, const uint32_t* snapshot, void* stream) {
    MAEST_REQUIRE(x && delta && x_out && gamma && beta && y, "maest_drop_add_layernorm_fwd: null pointer");
    MAEST_REQUIRE((y_dtype == MAEST_F32 || y_dtype == MAEST_BF16) && (delta_dtype == MAEST_F32 || delta_dtype == MAEST_BF16),
                  "maest_drop_add_layernorm_fwd: bad dtype");
    if (!drop_args_ok("maest_drop_add_layernorm_fwd", B, N, n_rows_per_clip, cols, site_e, site_p, snapshot)) return MAEST_ERR_INVALID;
    const int rows = B * n_rows_per_clip;
    DropArgs a{snapshot, N, n_rows_per_clip, site_e, thr_e, scale_e, site_p, thr_p, scale_p};
    hipLaunchKernelGGL((drop_row_kernel<true, false>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, delta, delta_dtype, x_out,
                       gamma, beta, y, y_dtype, mean, rstd, rows, eps, a);
    return check_launch("maest_drop_add_layernorm_fwd");
}

extern "C" int maest_drop_add(const float* x, const void* delta, int delta_dtype, float* x_out, int B, int N, int n_rows_per_clip,
                              int cols, int site_e, uint32_t thr_e, float scale_e, int site_p, uint32_t thr_p, float scale_p,
                              const uint32_t* snapshot, void* stream) {
    MAEST_REQUIRE(x && delta && x_out, "maest_drop_add: null pointer");
    MAEST_REQUIRE(delta_dtype == MAEST_F32 || delta_dtype == MAEST_BF16, "maest_drop_add: bad dtype");
    if (!drop_args_ok("maest_drop_add", B, N, n_rows_per_clip, cols, site_e, site_p, snapshot)) return MAEST_ERR_INVALID;
    const int rows = B * n_rows_per_clip;
    DropArgs a{snapshot, N, n_rows_per_clip, site_e, thr_e, scale_e, site_p, thr_p, scale_p};
    hipLaunchKernelGGL((drop_row_kernel<false, false>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, delta, delta_dtype, x_out,
                       (const float*)nullptr, (const float*)nullptr, (void*)nullptr, MAEST_F32, (float*)nullptr, (float*)nullptr, rows, 0.0f, a);
    return check_launch("maest_drop_add");
}

extern "C" int maest_drop_cast(const float* src, void* dst, int dst_dtype, int B, int N, int n_rows_per_clip, int cols, int site_e,
                               uint32_t thr_e, float scale_e, int site_p, uint32_t thr_p, float scale_p, const uint32_t* snapshot,
                               void* stream) {
    MAEST_REQUIRE(src && dst, "maest_drop_cast: null pointer");
    MAEST_REQUIRE(dst_dtype == MAEST_F32 || dst_dtype == MAEST_BF16, "maest_drop_cast: bad dtype");
    MAEST_REQUIRE((const void*)src != (const void*)dst, "maest_drop_cast: dst must not alias src (the residual stream's gradient passes unmodified)");
    if (!drop_args_ok("maest_drop_cast", B, N, n_rows_per_clip, cols, site_e, site_p, snapshot)) return MAEST_ERR_INVALID;
    const int rows = B * n_rows_per_clip;
    DropArgs a{snapshot, N, n_rows_per_clip, site_e, thr_e, scale_e, site_p, thr_p, scale_p};
    hipLaunchKernelGGL((drop_row_kernel<false, true>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, (const void*)nullptr,
                       MAEST_F32, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, dst, dst_dtype, (float*)nullptr,
                       (float*)nullptr, rows, 0.0f, a);
    return check_launch("maest_drop_cast");
}
