// Fused log-mel front end: reflect-padded framing -> Hann window -> 512-point real FFT -> |.|^2 ->
// 96-band slaney mel projection -> log10(1 + 1e4 x) -> z-norm, one kernel, one HBM round trip.
// (reference: MelSpectrogram.forward models/helpers/melspectrogram.py:47-60 with the torchaudio
//  Spectrogram(n_fft=512, hop=256, power=2, center=True/reflect) :29-34 and MelScale(96, slaney) :36-42;
//  constants :16-24.)
//
// Algorithmically HBM-bound (0.88 MB / 10 s clip in+out vs ~7 MFLOP of FFT); instruction-issue bound as written.  A
// workgroup owns 64 consecutive frames of one clip so that the [96, T] output is written as 256-byte runs along T; each of
// its 4 waves transforms 16 frames, FOUR at a time (16 lanes per frame, 16 complex points per lane; the next four frames'
// samples in flight), without block barriers: the 512 real samples are packed as 256 complex points and transformed as
// 256 = 16 x 16 -- two 16-point DFTs in registers around one exchange through LDS --, unpacked to the 257-bin one-sided
// spectrum, and projected onto the mel bands with the filterbank stored in band-sparse form (each triangular band touches
// <= fb_stride consecutive bins): the four frames' power spectra lie bin-major in LDS, a lane forms one band and one half
// band of all four frames from 16-byte reads with its weights in registers.  All arithmetic is fp32.  (Rounds 1-2: one
// frame per wave, four radix-4 stages through LDS, ~800 instructions per frame and wave = 0.11 of the HBM roofline; round 3:
// 16 x 16 with a per-frame projection, ~440 = 0.17; round 5: the projection over four frames at once, ~280 = 0.23, then the FFT
// stages and the unpack in packed fp32 instructions with explicit operand modifiers, ~165 = 0.31 -- DESIGN.md section 4.)
#include <type_traits>

#include "common.h"

namespace maest {

constexpr int MEL_NFFT = 512;
constexpr int MEL_HOP = 256;
constexpr int MEL_NBINS = 257;
constexpr int MEL_BANDS = 96;
constexpr int MEL_FRAMES_PER_BLOCK = 64;
constexpr int MEL_OUT_LD = MEL_FRAMES_PER_BLOCK + 1;

// A complex value is a (re, im) pair in ONE 64-bit register pair, and the arithmetic is the packed fp32 instruction set with its operand
// modifiers written out: `op_sel` / `op_sel_hi` choose which half of a source feeds the low / high result, `neg_lo` / `neg_hi` negate it --
// a multiplication by -i or a conjugation costs no instruction, a complex product two.  (Left to hipcc, the same source spent a third of
// the two 16-point DFT stages on moves that re-paired registers: 175 of 518 instructions per four frames.)  The host emulator takes the
// plain C++ twins, which perform the same IEEE operations.
typedef f32x2_t cplx;
#define MEL_RE(z) ((z)[0])
#define MEL_IM(z) ((z)[1])
#if defined(__AMDGCN__)
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { cplx d; asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { cplx d; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
// a + (-i) t = (a.re + t.im, a.im - t.re)  /  a - (-i) t = (a.re - t.im, a.im + t.re)
__device__ __forceinline__ cplx cadd_rot(cplx a, cplx t) { cplx d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(t)); return d; }
__device__ __forceinline__ cplx csub_rot(cplx a, cplx t) { cplx d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(d) : "v"(a), "v"(t)); return d; }
// a b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re): the a.im products first (cmul_a), then a.re (b.re, b.im) added by one packed fma (cmul_b)
// (the two halves of a product as separate statements: asm statements keep their source order, so independent products are written
//  interleaved -- first halves, then second halves -- and no instruction waits on its predecessor)
template <bool NEG>
__device__ __forceinline__ cplx cmul_a(cplx a, cplx b) {         // NEG: the product with -b
    cplx t;
    if (NEG) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));  // (a.im b.im, -a.im b.re)
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    return t;
}
template <bool NEG>
__device__ __forceinline__ cplx cmul_b(cplx a, cplx b, cplx t) {
    cplx d;
    if (NEG) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0] neg_hi:[0,1,0]" : "=v"(d) : "v"(a), "v"(b), "v"(t));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(d) : "v"(a), "v"(b), "v"(t));
    return d;
}
// a + conj(p) / a - conj(p)
__device__ __forceinline__ cplx cadd_conj(cplx a, cplx p) { cplx d; asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(p)); return d; }
__device__ __forceinline__ cplx csub_conj(cplx a, cplx p) { cplx d; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(d) : "v"(a), "v"(p)); return d; }
__device__ __forceinline__ cplx csqr2(cplx a) { cplx q; asm("v_pk_mul_f32 %0, %1, %1" : "=v"(q) : "v"(a)); return q; }      // (re^2, im^2)
#else
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return cplx{a[0] + b[0], a[1] + b[1]}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return cplx{a[0] - b[0], a[1] - b[1]}; }
__device__ __forceinline__ cplx cadd_rot(cplx a, cplx t) { return cplx{a[0] + t[1], a[1] - t[0]}; }
__device__ __forceinline__ cplx csub_rot(cplx a, cplx t) { return cplx{a[0] - t[1], a[1] + t[0]}; }
template <bool NEG>
__device__ __forceinline__ cplx cmul_a(cplx a, cplx b) { return NEG ? cplx{a[1] * b[1], -(a[1] * b[0])} : cplx{-(a[1] * b[1]), a[1] * b[0]}; }
template <bool NEG>
__device__ __forceinline__ cplx cmul_b(cplx a, cplx b, cplx t) {
    return NEG ? cplx{__builtin_fmaf(a[0], -b[0], t[0]), __builtin_fmaf(a[0], -b[1], t[1])}
               : cplx{__builtin_fmaf(a[0], b[0], t[0]), __builtin_fmaf(a[0], b[1], t[1])};
}
__device__ __forceinline__ cplx cadd_conj(cplx a, cplx p) { return cplx{a[0] + p[0], a[1] - p[1]}; }
__device__ __forceinline__ cplx csub_conj(cplx a, cplx p) { return cplx{a[0] - p[0], a[1] + p[1]}; }
__device__ __forceinline__ cplx csqr2(cplx a) { return cplx{a[0] * a[0], a[1] * a[1]}; }
#endif
__device__ __forceinline__ int rev4_256(int k) {  // reverse the four base-4 digits of k
    return ((k & 3) << 6) | (((k >> 2) & 3) << 4) | (((k >> 4) & 3) << 2) | ((k >> 6) & 3);
}

__device__ __forceinline__ float mel_log2(float x) { return __builtin_amdgcn_logf(x); }       // v_log_f32

// The value lane (16 - l) mod 16 of the same 16-lane row holds (l = lane mod 16) = mirror(next(x)): two DPP moves on the device -- rotate the
// row by one, mirror it: no LDS crossbar, no wait --, lane permutations under the host emulator.  (Two functions: a DPP move wants its source
// written two instructions earlier, so the callers issue them in batches.)
__device__ __forceinline__ float mel_row_next(float x, int lane) {          // the value of lane (l + 1) mod 16
#if defined(__AMDGCN__)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x12f /* row_ror:15 */, 0xf, 0xf, false));
#else
    return __shfl(x, (lane & 48) | ((lane + 1) & 15), 64);
#endif
}
__device__ __forceinline__ float mel_row_mirror(float x, int lane) {        // the value of lane 15 - l
#if defined(__AMDGCN__)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x140 /* row_mirror */, 0xf, 0xf, false));
#else
    return __shfl(x, (lane & 48) | (15 - (lane & 15)), 64);
#endif
}

__device__ __forceinline__ float mel_lane_xor1(float x) {                   // the value of lane ^ 1
#if defined(__AMDGCN__)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xb1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false));
#else
    return __shfl_xor(x, 1, 64);
#endif
}

// LDS hand-off between the lanes of ONE wave: a wave's DS instructions execute in order and all 64 lanes issue them
// together, so a write by one lane is visible to a later read by another lane of the same wave without a barrier;
// only the compiler has to keep the order (the host emulator, one thread per lane, maps this to a wave barrier).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- 16-point DFT in registers: v[n] (n = 4 a + b) -> Y[k] (k = c + 4 d) left at v[4 c + d] (base-4 digit reversal).  Four radix-4
// butterflies at a time, written operation by operation across the four (no statement depends on the one in front of it).
// ROT2 (second stage, third butterfly): its third input still owes a factor -i (the twiddle exp(-2 pi i 4 / 16)), taken by operand modifiers.
template <int S0, int ST, bool STAGE2>      // butterfly j works on v[S0 j + ST i], i = 0 .. 3
__device__ __forceinline__ void dft4x4(cplx (&v)[16]) {
    cplx b0[4], b1[4], b2[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool rot = STAGE2 && j == 2;
        b0[j] = rot ? cadd_rot(v[S0 * j], v[S0 * j + 2 * ST]) : cadd(v[S0 * j], v[S0 * j + 2 * ST]);
        b2[j] = cadd(v[S0 * j + ST], v[S0 * j + 3 * ST]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool rot = STAGE2 && j == 2;
        b1[j] = rot ? csub_rot(v[S0 * j], v[S0 * j + 2 * ST]) : csub(v[S0 * j], v[S0 * j + 2 * ST]);
        t[j] = csub(v[S0 * j + ST], v[S0 * j + 3 * ST]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[S0 * j] = cadd(b0[j], b2[j]);
        v[S0 * j + 2 * ST] = csub(b0[j], b2[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[S0 * j + ST] = cadd_rot(b1[j], t[j]);
        v[S0 * j + 3 * ST] = csub_rot(b1[j], t[j]);
    }
}
__device__ __forceinline__ void dft16(cplx (&v)[16]) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R = 0.70710678118654752f;
    const cplx w1 = {C1, -S1}, w2 = {R, -R}, w3 = {S1, -C1}, w6 = {R, R};
    dft4x4<1, 4, false>(v);                            // over a: v[4 c + b] = T[c][b]
    // T[c][b] *= exp(-2 pi i b c / 16)   (b c = 4: -i, left to the second stage's butterfly; -(R, R) and -(C1, -S1) by operand modifiers)
    const cplx t5 = cmul_a<false>(v[5], w1), t9 = cmul_a<false>(v[9], w2), t13 = cmul_a<false>(v[13], w3), t6 = cmul_a<false>(v[6], w2);
    const cplx t14 = cmul_a<true>(v[14], w6), t7 = cmul_a<false>(v[7], w3), t11 = cmul_a<true>(v[11], w6), t15 = cmul_a<true>(v[15], w1);
    v[5] = cmul_b<false>(v[5], w1, t5); v[9] = cmul_b<false>(v[9], w2, t9); v[13] = cmul_b<false>(v[13], w3, t13); v[6] = cmul_b<false>(v[6], w2, t6);
    v[14] = cmul_b<true>(v[14], w6, t14); v[7] = cmul_b<false>(v[7], w3, t7); v[11] = cmul_b<true>(v[11], w6, t11); v[15] = cmul_b<true>(v[15], w1, t15);
    dft4x4<4, 1, true>(v);                             // over b: v[4 c + d] = Y[c + 4 d]
}
__device__ __forceinline__ constexpr int rev16(int k) { return 4 * (k & 3) + (k >> 2); }    // where dft16 leaves Y[k]

// the 16 complex points (= 32 samples) of frame t that lane l of a 16-lane group packs: z[16 n1 + l], n1 = 0..15.
// INTERIOR (block-uniform: all 64 frames of the block lie inside the clip and the clip starts 8-byte aligned): plain 8-byte
// loads, 16 lanes = one 128-byte line; otherwise clamped (frames >= T take the last frame's data and are not stored) and
// reflect-padded sample by sample
template <bool INTERIOR>
__device__ __forceinline__ void mel_fetch(cplx (&xin)[16], const float* __restrict__ wsrc, int t, int T, int S, int l) {
    if (INTERIOR) {
        const float* p0 = wsrc + t * MEL_HOP - MEL_NFFT / 2 + 2 * l;
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            xin[n1] = *reinterpret_cast<const cplx*>(p0 + 32 * n1);
        }
        return;
    }
    const int tc = t < T ? t : T - 1;
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
        const int p = 2 * (16 * n1 + l);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int i = tc * MEL_HOP + p + e - MEL_NFFT / 2;
            if (i < 0) i = -i;
            if (i >= S) i = 2 * (S - 1) - i;
            xin[n1][e] = wsrc[i];
        }
    }
}

constexpr int MEL_XROW = 18 * 8;                  // exchange tile: 16 rows (k1) of 16 complex, pitch 18 (b128 reads conflict-free)
constexpr int MEL_XFRAME = 16 * MEL_XROW;         // 2304 B per frame
constexpr int MEL_PWBINS = 272;                   // 257 bins + 15 zero bins (a 16-weight register window starting at the last band's first bin)

// Where a block's [96][64] output tile goes (the only part of the block that differs between the two entries):
//   MelEpiBandMajor -- maest_logmel: fp32 [B, 96, T], 256-byte runs along T;
//   MelEpiRowsF16   -- maest_logmel_rows_f16: IEEE half rows [frame][96] (the on-disk mel file's layout), the block's frames one
//                      contiguous run of up to 64 x 192 bytes, stored 16 bytes per thread.
struct MelEpiBandMajor {
    float* __restrict__ out;         // [B, 96, T]
    int b = 0;                       // the block's clip
    __device__ __forceinline__ const float* locate(const float* wave_in, int& S, int&, int& t0) {      // grid (T / 64, B)
        b = blockIdx.y;
        t0 = blockIdx.x * MEL_FRAMES_PER_BLOCK;
        return wave_in + (int64_t)b * S;
    }
    __device__ __forceinline__ void store(const float* otile, int t0, int T) const {
        const int tl = threadIdx.x & 63, m0 = threadIdx.x >> 6;       // thread = frame tid & 63 of bands (tid >> 6) + 4 j
        if (t0 + tl < T) {
            float* dst = out + ((int64_t)b * MEL_BANDS + m0) * T + t0 + tl;
            const float* src = otile + m0 * MEL_OUT_LD + tl;
#pragma unroll
            for (int j = 0; j < MEL_BANDS / 4; ++j) dst[(int64_t)4 * j * T] = src[4 * j * MEL_OUT_LD];
        }
    }
};
typedef _Float16 mel_h8_t __attribute__((ext_vector_type(8)));
constexpr int MEL_TRACK_FIELDS = 5;      // maest_logmel_rows_f16's track table: sample offset, S, first frame f0, frame count n, row offset
struct MelEpiRowsF16 {
    const int64_t* __restrict__ tracks;          // [n_tracks][5]
    const int32_t* __restrict__ block_start;     // [n_tracks + 1]: first block of each track, ceil(n / 64) blocks per track
    int n_tracks;
    int64_t total_in, total_rows;                // the packed input's samples, the packed output's rows
    _Float16* __restrict__ rows_out;             // [total_rows][96]
    _Float16* rows = nullptr;                    // the row of the block's first frame
    int n_rows = 0;                              // frames of the block that are stored (<= 64)
    // grid (block_start[n_tracks]): the block's track by bisection; a table entry outside the buffers stores nothing (and reads inside them)
    __device__ __forceinline__ const float* locate(const float* wave_in, int& S, int& T, int& t0) {
        const int bid = blockIdx.x;
        int lo = 0, hi = n_tracks - 1;          // the last track whose first block is <= bid
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (block_start[mid] <= bid) lo = mid;
            else hi = mid - 1;
        }
        const int64_t* tr = tracks + MEL_TRACK_FIELDS * lo;
        const int64_t off = tr[0], s = tr[1], f0 = tr[2], n = tr[3], r0 = tr[4];
        const int64_t j = bid - block_start[lo];
        const bool ok = s > MEL_NFFT / 2 && s <= INT32_MAX - 4 * MEL_NFFT && off >= 0 && off + s <= total_in && f0 >= 0 && n >= 1 &&
                        f0 + n <= 1 + s / MEL_HOP && r0 >= 0 && r0 + n <= total_rows && j >= 0 && MEL_FRAMES_PER_BLOCK * j < n;
        if (!ok) {
            S = (int)(total_in < INT32_MAX - 4 * MEL_NFFT ? total_in : INT32_MAX - 4 * MEL_NFFT);
            T = 1 + S / MEL_HOP;
            t0 = 0;
            return wave_in;
        }
        S = (int)s;
        T = 1 + S / MEL_HOP;
        t0 = (int)(f0 + MEL_FRAMES_PER_BLOCK * j);
        const int64_t left = n - MEL_FRAMES_PER_BLOCK * j;
        n_rows = left < MEL_FRAMES_PER_BLOCK ? (int)left : MEL_FRAMES_PER_BLOCK;
        rows = rows_out + (r0 + MEL_FRAMES_PER_BLOCK * j) * MEL_BANDS;
        return wave_in + off;
    }
    __device__ __forceinline__ void store(const float* otile, int, int) const {
        // 12 chunks of 8 bands per frame: chunk c = frame c / 12, bands 8 (c % 12) .. + 7 -- consecutive threads, consecutive 16 bytes
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int c = threadIdx.x + 256 * r;
            const int f = c / 12, m0 = 8 * (c - 12 * f);
            if (f < n_rows) {
                mel_h8_t h;
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = (_Float16)otile[(m0 + i) * MEL_OUT_LD + f];      // round to nearest even
                *reinterpret_cast<mel_h8_t*>(rows + 8 * c) = h;
            }
        }
    }
};

// Round 3 form: a wave transforms FOUR frames at a time, 16 lanes per frame and 16 complex points per lane, as 256 = 16 x 16:
// a 16-point DFT over n1 in registers (twiddles of the 16-point transform are literals), the W256^(n2 k1) factors (per-lane
// registers), ONE exchange through LDS (lane n2 writes column n2, lane k1 reads row k1), a 16-point DFT over n2 in registers.
// The real-FFT unpack needs Z[256 - k], which lives in lane 16 - l of the same group: one lane permutation per value.  The
// mel projection runs over the four frames at once (a band and a half band per lane, filter weights in registers).  Per frame and
// wave ~165 instructions (counted in the code object: ~650 per four frames) against ~800 for four radix-4 stages through LDS with
// one frame per wave.
// EPI::locate finds the block's clip, its first frame t0 and (in a ragged batch) the clip's S and T; EPI::store writes the tile
template <class EPI>
__global__ __launch_bounds__(256, 2) void logmel_kernel(const float* __restrict__ wave_in, int S, int T,
                                                     const float* __restrict__ window,
                                                     const float* __restrict__ twiddle,   // [512][2] exp(-2 pi i k / 512)
                                                     const int32_t* __restrict__ fb_start,
                                                     const int32_t* __restrict__ fb_len,
                                                     const float* __restrict__ fb_w, int fb_stride, float log_scale,
                                                     float norm_mean, float norm_2std, EPI epi) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l = lane & 15, grp = lane >> 4;
    float* wtab = reinterpret_cast<float*>(smem);                     // [512] Hann window
    float* tw256 = wtab + 512;                                        // [16 k1][16 l][2] exp(-2 pi i l k1 / 256): lane l reads at l + 16 k1 (immediate offsets)
    float* tw512 = tw256 + 512;                                       // [256][2] exp(-2 pi i k / 512): lane l reads at l + 16 k2
    float* otile = tw512 + 512;                                       // [96][65]
    char* xch = reinterpret_cast<char*>(otile + MEL_BANDS * MEL_OUT_LD) + wv * 4 * MEL_XFRAME;          // per wave: 4 frames
    // the power spectra of the four frames reuse the exchange tiles (2304 >= 1040 bytes per frame; a wave-level sync apart)
    int t0;
    const float* wsrc = epi.locate(wave_in, S, T, t0);
    const bool interior = t0 > 0 && (t0 + MEL_FRAMES_PER_BLOCK) * MEL_HOP + MEL_NFFT / 2 <= S && t0 + MEL_FRAMES_PER_BLOCK <= T &&
                          (reinterpret_cast<uintptr_t>(wsrc) & 7) == 0;      // block-uniform
    cplx xin[16];          // the lane's 16 packed points as loaded: (even, odd) sample = (re, im)
    // this lane's band (lane) and half band (64 + lane / 2, weight slots 8 (lane & 1) .. + 7): first bin, length
    const int mbnd = 64 + (lane >> 1);
    const int sa = fb_start[lane], na = fb_len[lane] < fb_stride ? fb_len[lane] : fb_stride;
    const int sb = fb_start[mbnd] + 8 * (lane & 1), nb = fb_len[mbnd] < fb_stride ? fb_len[mbnd] : fb_stride;
    // log10(1 + s x) -> z-norm as one multiply-add behind the hardware's log2 (v_log_f32, 1 ulp; the argument is >= 1)
    const float out_mul = 0.30102999566398120f / norm_2std, out_add = -norm_mean / norm_2std;
    const float ls4 = 0.25f * log_scale;         // the power spectra below are kept times four
    // tables: 128 threads copy the window, 128 the 512-point twiddles (16 bytes each), every thread gathers one 256-point twiddle
    if (threadIdx.x < 128) *reinterpret_cast<f32x4_t*>(wtab + 4 * threadIdx.x) = *reinterpret_cast<const f32x4_t*>(window + 4 * threadIdx.x);
    else *reinterpret_cast<f32x4_t*>(tw512 + 4 * (threadIdx.x - 128)) = *reinterpret_cast<const f32x4_t*>(twiddle + 4 * (threadIdx.x - 128));
    *reinterpret_cast<cplx*>(tw256 + 2 * threadIdx.x) =
        *reinterpret_cast<const cplx*>(twiddle + 4 * (((threadIdx.x & 15) * (threadIdx.x >> 4)) & 255));       // exp(-2 pi i l k1 / 256) at [16 k1 + l]
    // the first 8 filter weights of this lane's band and its half band's 8 (zero beyond the band: the host pads its rows with zeros)
    float wa[8], wb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wa[i] = i < na ? fb_w[lane * fb_stride + i] : 0.0f;
        wb[i] = 8 * (lane & 1) + i < nb ? fb_w[mbnd * fb_stride + 8 * (lane & 1) + i] : 0.0f;
    }
    __syncthreads();

    // (one copy of the frame loop per fetch form: with both forms inside one loop the prefetch registers met in phi copies, 32 moves per pass)
    auto frames = [&](auto interior_tag) {
        constexpr bool INTERIOR = decltype(interior_tag)::value;
        mel_fetch<INTERIOR>(xin, wsrc, t0 + wv * 16 + grp, T, S, l);
        for (int quad = 0; quad < 4; ++quad) {
            const int tl0 = wv * 16 + quad * 4;      // first of this wave's four frames within the block
            // ---- framing (center=True, reflect padding of 256 samples) + window + complex packing: v[n1] = z[16 n1 + l]
            cplx v[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const cplx w2 = *reinterpret_cast<const cplx*>(wtab + 2 * (16 * n1 + l));
                v[n1] = xin[n1] * w2;
            }
            if (quad + 1 < 4) {                       // the next four frames' samples fly while these are transformed
                mel_fetch<INTERIOR>(xin, wsrc, t0 + tl0 + 4 + grp, T, S, l);
            }
            // ---- 256 = 16 x 16: DFT over n1, twiddle, exchange, DFT over n2.  (The lane's table values are read a stage ahead of their use:
            // the packed-math statements are asm, which hipcc does not move loads across)
            cplx tw[15];
#pragma unroll
            for (int k1 = 1; k1 < 16; ++k1) tw[k1 - 1] = *reinterpret_cast<const cplx*>(tw256 + 2 * (16 * k1 + l));      // W256^(l k1)
            dft16(v);
            char* xf = xch + grp * MEL_XFRAME;
            *reinterpret_cast<cplx*>(xf + l * 8) = v[rev16(0)];
#pragma unroll
            for (int g = 0; g < 3; ++g) {             // k1 = 1 + 5 g .. 5 + 5 g: five products at a time, first halves then second halves
                cplx ta[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) ta[i] = cmul_a<false>(v[rev16(1 + 5 * g + i)], tw[5 * g + i]);
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    *reinterpret_cast<cplx*>(xf + (1 + 5 * g + i) * MEL_XROW + l * 8) = cmul_b<false>(v[rev16(1 + 5 * g + i)], tw[5 * g + i], ta[i]);
            }
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4_t q = *reinterpret_cast<const f32x4_t*>(xf + l * MEL_XROW + j * 16);
                v[2 * j] = cplx{q[0], q[1]};
                v[2 * j + 1] = cplx{q[2], q[3]};
            }
            cplx wu[16];
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) wu[k2] = *reinterpret_cast<const cplx*>(tw512 + 2 * (l + 16 * k2));          // exp(-2 pi i (l + 16 k2) / 512)
            dft16(v);                                 // Z[l + 16 k2] at v[rev16(k2)]
            // ---- unpack the real FFT: X[k] = E[k] + W512^k O[k], power spectrum for k = l + 16 k2 (and bin 256 from lane 0)
            wave_lds_sync();                          // every lane has read its row: the tiles become the power spectra
            // power spectra of the wave's four frames, bin-major: pw[bin][frame] -- the projection below takes one bin of all four frames
            // with a single 16-byte read; the 64 lanes of a store cover 64 consecutive floats.  Bins 257 .. 271 are zero: a band's
            // register-resident weights run past its last bin (weight 0) and must meet finite values there.
            float* pw = reinterpret_cast<float*>(xch);
            if (lane < 4 * (MEL_PWBINS - MEL_NBINS)) pw[4 * MEL_NBINS + lane] = 0.0f;
                // Z[256 - k] sits in lane 16 - l, slot 15 - k2 (lane 0 pairs with itself: slot (16 - k2) mod 16): the partner values of all 16 slots
            // first (selects and lane moves: plain statements, scheduled by hipcc), then the packed arithmetic four slots at a time
            cplx pz[16];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {          // eight slots at a time: selects, then the rotations, then the mirrors
                float sr[8], si[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int k2 = 8 * hf + i;
                    const cplx za = v[rev16((16 - k2) & 15)], zb = v[rev16(15 - k2)];      // (selected per component: a select between
                    sr[i] = l == 0 ? MEL_RE(za) : MEL_RE(zb);                               //  two array elements would pin v[] to scratch)
                    si[i] = l == 0 ? MEL_IM(za) : MEL_IM(zb);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) { sr[i] = mel_row_next(sr[i], lane); si[i] = mel_row_next(si[i], lane); }
#pragma unroll
                for (int i = 0; i < 8; ++i) pz[8 * hf + i] = cplx{mel_row_mirror(sr[i], lane), mel_row_mirror(si[i], lane)};
            }
            if (l == 0) {
                const float x256 = 2.0f * (MEL_RE(v[rev16(0)]) - MEL_IM(v[rev16(0)]));      // 2 X[256] = 2 (Re Z[0] - Im Z[0])
                pw[4 * 256 + grp] = x256 * x256;
            }
            // 2 X[k] = (Z[k] + conj Z[N-k]) - i (Z[k] - conj Z[N-k]) W512^k: the halves are left out (the power comes out times four,
            // exactly; the factor rides in the log's scale below)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                cplx e[4], d[4], t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { e[i] = cadd_conj(v[rev16(4 * g + i)], pz[4 * g + i]); d[i] = csub_conj(v[rev16(4 * g + i)], pz[4 * g + i]); }
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = cmul_a<false>(d[i], wu[4 * g + i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = cmul_b<false>(d[i], wu[4 * g + i], t[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) e[i] = cadd_rot(e[i], d[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = csqr2(e[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) pw[4 * (l + 16 * (4 * g + i)) + grp] = MEL_RE(t[i]) + MEL_IM(t[i]);
            }
            wave_lds_sync();
            // ---- mel projection + logC + z-norm into the block's output tile, the wave's four frames at once: lane L forms band L from
            // 8 bins (the slaney bank's bands 0 .. 63 are 1 .. 6 bins long) and one HALF of band 64 + L / 2 (8 of its 16 weight slots: bands
            // 64 .. 95 are 6 .. 15 bins long), a bin of the four frames per 16-byte LDS read, the weights in registers (wa / wb, loaded in
            // front of the frame loop); the halves meet through one lane exchange.  Longer bands finish in a global-read loop (never with
            // this bank).  (Rounds 3 - 5a: one frame at a time, 1.5 bands per lane, a 4-byte LDS read per product and its wait in front of
            // every multiply-add: 724 of the ~1800 instructions a wave spent on four frames.)
            {
                const f32x4_t* pwq = reinterpret_cast<const f32x4_t*>(xch);
                f32x4_t acc_a = {0.0f, 0.0f, 0.0f, 0.0f}, acc_b = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const f32x4_t pa = pwq[sa + i], pb = pwq[sb + i];
                    acc_a = __builtin_elementwise_fma(pa, f32x4_t{wa[i], wa[i], wa[i], wa[i]}, acc_a);
                    acc_b = __builtin_elementwise_fma(pb, f32x4_t{wb[i], wb[i], wb[i], wb[i]}, acc_b);
                }
#pragma unroll 1
                for (int i = 8; i < na; ++i) acc_a += pwq[sa + i] * fb_w[lane * fb_stride + i];
#pragma unroll
                for (int f = 0; f < 4; ++f) acc_b[f] += mel_lane_xor1(acc_b[f]);
                if ((lane & 1) == 0)
#pragma unroll 1
                    for (int i = 16; i < nb; ++i) acc_b += pwq[sb + i] * fb_w[mbnd * fb_stride + i];
                const int tl = wv * 16 + quad * 4;
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    otile[lane * MEL_OUT_LD + tl + f] = __builtin_fmaf(mel_log2(__builtin_fmaf(acc_a[f], ls4, 1.0f)), out_mul, out_add);
                    if ((lane & 1) == 0)
                        otile[mbnd * MEL_OUT_LD + tl + f] = __builtin_fmaf(mel_log2(__builtin_fmaf(acc_b[f], ls4, 1.0f)), out_mul, out_add);
                }
            }
            wave_lds_sync();       // pw / the exchange tile are rewritten by the next four frames
        }
    };
    if (interior) frames(std::true_type{});
    else frames(std::false_type{});
    __syncthreads();
    epi.store(otile, t0, T);           // ---- coalesced store of the [96][64] tile
}


// ---------------------------------------------------------------------------------------------------------------------------------------
// Backward of logmel_kernel: dwave from g = dL/dout.  Per frame t (fp32 throughout; X = the frame's one-sided spectrum, recomputed here
// rather than saved: it is as large as the waveform):
//   dmel[m] = g[m] log_scale / (ln 10 norm_2std (1 + log_scale mel[m]))         (1 + s mel >= 1: bounded)
//   dP[k]   = sum_m fb[k, m] dmel[m]                                            (a bin lies in <= 2 bands: per-bin table, no scatter)
//   dz[n]   = sum_{k=0}^{256} 2 dP[k] Re(X[k] exp(+2 pi i k n / 512))           = the real inverse DFT of the Hermitian H with
//             H[k] = dP[k] X[k] (k = 1 .. 255), H[0] = 2 dP[0] X[0], H[256] = 2 dP[256] X[256]  (bins 0 and 256 have no mirror)
//   dframe[n] = win[n] dz[n]
// then overlap-add at hop 256 with the reflect padding folded back.  Two kernels: logmel_bwd_frames_kernel writes
// dframe for every frame to an fp32 scratch [B, T, 512]; logmel_bwd_gather_kernel gives each sample ONE thread that adds its (at most
// four) contributions in a fixed order -- deterministic, no atomics.
//
// The inverse transform is the forward one run backwards: with Hc = conj H and its mirror partner taken by the forward unpack's lane
// moves, the unpack expression yields conj(Zi[k]), Zi[k] = (H[k] + conj H[256 - k]) + i (H[k] - conj H[256 - k]) exp(+2 pi i k / 512)
// (k = 0 pairs with H[256]); the same 256-point DFT of conj(Zi) is conj(x_even + i x_odd).

// the group's 256-point DFT: v[n1] = z[16 n1 + l] in, Z[l + 16 k2] at v[k2] out (plain slot order); xf: the group's exchange tile.  The
// exchange tile (and whatever shares the wave's LDS with it) is free again on return.
__device__ __forceinline__ void mel_fft256(cplx (&v)[16], char* xf, const float* tw256, int l) {
    cplx tw[15];
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) tw[k1 - 1] = *reinterpret_cast<const cplx*>(tw256 + 2 * (16 * k1 + l));      // W256^(l k1)
    dft16(v);
    *reinterpret_cast<cplx*>(xf + l * 8) = v[rev16(0)];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        cplx ta[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) ta[i] = cmul_a<false>(v[rev16(1 + 5 * g + i)], tw[5 * g + i]);
#pragma unroll
        for (int i = 0; i < 5; ++i)
            *reinterpret_cast<cplx*>(xf + (1 + 5 * g + i) * MEL_XROW + l * 8) = cmul_b<false>(v[rev16(1 + 5 * g + i)], tw[5 * g + i], ta[i]);
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4_t q = *reinterpret_cast<const f32x4_t*>(xf + l * MEL_XROW + j * 16);
        v[2 * j] = cplx{q[0], q[1]};
        v[2 * j + 1] = cplx{q[2], q[3]};
    }
    dft16(v);
    cplx o[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) o[k2] = v[rev16(k2)];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) v[k2] = o[k2];
    wave_lds_sync();
}

// pz[k2] = the value at slot 256 - k of the group, k = l + 16 k2: lane (16 - l) mod 16, slot 15 - k2 (lane 0: its own slot (16 - k2) mod 16;
// for k = 0 that is slot 0 itself, which the caller replaces where 256 is meant) -- the forward unpack's lane moves
__device__ __forceinline__ void mel_mirror_partners(const cplx (&z)[16], cplx (&pz)[16], int lane) {
    const int l = lane & 15;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        float sr[8], si[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k2 = 8 * hf + i;
            const cplx za = z[(16 - k2) & 15], zb = z[15 - k2];
            sr[i] = l == 0 ? MEL_RE(za) : MEL_RE(zb);
            si[i] = l == 0 ? MEL_IM(za) : MEL_IM(zb);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { sr[i] = mel_row_next(sr[i], lane); si[i] = mel_row_next(si[i], lane); }
#pragma unroll
        for (int i = 0; i < 8; ++i) pz[8 * hf + i] = cplx{mel_row_mirror(sr[i], lane), mel_row_mirror(si[i], lane)};
    }
}

// out[k2] = (z + conj pz) - i (z - conj pz) wu  per slot: 2 X[k] from Z (forward), conj(Zi[k]) from conj H (backward)
__device__ __forceinline__ void mel_unpack(const cplx (&z)[16], const cplx (&pz)[16], const float* tw512, int l, cplx (&out)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        cplx e[4], d[4], t[4], wu[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wu[i] = *reinterpret_cast<const cplx*>(tw512 + 2 * (l + 16 * (4 * g + i)));      // exp(-2 pi i k / 512)
#pragma unroll
        for (int i = 0; i < 4; ++i) { e[i] = cadd_conj(z[4 * g + i], pz[4 * g + i]); d[i] = csub_conj(z[4 * g + i], pz[4 * g + i]); }
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = cmul_a<false>(d[i], wu[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = cmul_b<false>(d[i], wu[i], t[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[4 * g + i] = cadd_rot(e[i], d[i]);
    }
}

constexpr int MELB_DMEL_OFF = 4 * MEL_PWBINS * 4;       // per wave: dmel [96 bands][4 frames] behind the power spectra (bytes)
static_assert(MELB_DMEL_OFF + MEL_BANDS * 16 <= 4 * MEL_XFRAME, "logmel_bwd: the wave's LDS");

// A wave takes four frames at a time (16 lanes per frame, as the forward); a block 64 frames of one clip.
__global__ __launch_bounds__(256, 2) void logmel_bwd_frames_kernel(const float* __restrict__ wave_in, int S, int T,
                                                                const float* __restrict__ window,
                                                                const float* __restrict__ twiddle,
                                                                const int32_t* __restrict__ fb_start,
                                                                const int32_t* __restrict__ fb_len,
                                                                const float* __restrict__ fb_w, int fb_stride,
                                                                const int32_t* __restrict__ bin_band,   // [257][2]
                                                                const float* __restrict__ bin_w,        // [257][2]
                                                                const float* __restrict__ grad_out,     // [B, 96, T]
                                                                float log_scale, float norm_2std,
                                                                float* __restrict__ dframes) {          // [B, T, 512]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l = lane & 15, grp = lane >> 4;
    float* wtab = reinterpret_cast<float*>(smem);                     // [512] Hann window
    float* tw256 = wtab + 512;                                        // [16 k1][16 l][2] exp(-2 pi i l k1 / 256)
    float* tw512 = tw256 + 512;                                       // [256][2] exp(-2 pi i k / 512)
    int32_t* bband = reinterpret_cast<int32_t*>(tw512 + 512);         // [257][2] the bands of each bin (4 * band: float offsets into dmel)
    float* bwt = tw512 + 512 + 2 * 260;                               // [257][2] their weights
    char* xch = reinterpret_cast<char*>(bwt + 2 * 260) + wv * 4 * MEL_XFRAME;
    float* pw = reinterpret_cast<float*>(xch);                        // [272 bins][4 frames]
    f32x4_t* dml = reinterpret_cast<f32x4_t*>(xch + MELB_DMEL_OFF);    // [96 bands][4 frames]
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * MEL_FRAMES_PER_BLOCK;
    const float* wsrc = wave_in + (int64_t)b * S;
    const float* gsrc = grad_out + (int64_t)b * MEL_BANDS * T;
    const bool interior = t0 > 0 && (t0 + MEL_FRAMES_PER_BLOCK) * MEL_HOP + MEL_NFFT / 2 <= S && t0 + MEL_FRAMES_PER_BLOCK <= T &&
                          (reinterpret_cast<uintptr_t>(wsrc) & 7) == 0;      // block-uniform
    const int mbnd = 64 + (lane >> 1);
    const int sa = fb_start[lane], na = fb_len[lane] < fb_stride ? fb_len[lane] : fb_stride;
    const int sb = fb_start[mbnd] + 8 * (lane & 1), nb = fb_len[mbnd] < fb_stride ? fb_len[mbnd] : fb_stride;
    const float ls4 = 0.25f * log_scale;
    const float dcoef = log_scale / (2.30258509299404568f * norm_2std);     // d out / d mel = dcoef / (1 + s mel)
    if (threadIdx.x < 128) *reinterpret_cast<f32x4_t*>(wtab + 4 * threadIdx.x) = *reinterpret_cast<const f32x4_t*>(window + 4 * threadIdx.x);
    else *reinterpret_cast<f32x4_t*>(tw512 + 4 * (threadIdx.x - 128)) = *reinterpret_cast<const f32x4_t*>(twiddle + 4 * (threadIdx.x - 128));
    *reinterpret_cast<cplx*>(tw256 + 2 * threadIdx.x) =
        *reinterpret_cast<const cplx*>(twiddle + 4 * (((threadIdx.x & 15) * (threadIdx.x >> 4)) & 255));
    for (int i = threadIdx.x; i < 2 * MEL_NBINS; i += 256) {
        bband[i] = 4 * bin_band[i];
        bwt[i] = bin_w[i];
    }
    float wa[8], wb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wa[i] = i < na ? fb_w[lane * fb_stride + i] : 0.0f;
        wb[i] = 8 * (lane & 1) + i < nb ? fb_w[mbnd * fb_stride + 8 * (lane & 1) + i] : 0.0f;
    }
    __syncthreads();

    auto frames = [&](auto interior_tag) {
        constexpr bool INTERIOR = decltype(interior_tag)::value;
        for (int quad = 0; quad < 4; ++quad) {
            const int tl0 = wv * 16 + quad * 4;      // first of this wave's four frames within the block
            const int t = t0 + tl0 + grp;            // this lane group's frame (>= T: clamped fetch, zero gradient, not stored)
            // ---- the forward, recomputed: framing + window, 256-point DFT, unpack to 2 X[k] (k = l + 16 k2 at xs[k2]; 2 X[256] in lane 0)
            cplx v[16];
            {
                cplx xin[16];
                mel_fetch<INTERIOR>(xin, wsrc, t, T, S, l);
#pragma unroll
                for (int n1 = 0; n1 < 16; ++n1) v[n1] = xin[n1] * *reinterpret_cast<const cplx*>(wtab + 2 * (16 * n1 + l));
            }
            mel_fft256(v, xch + grp * MEL_XFRAME, tw256, l);
            if (lane < 4 * (MEL_PWBINS - MEL_NBINS)) pw[4 * MEL_NBINS + lane] = 0.0f;
            cplx xs[16];
            float x256;
            {
                cplx pz[16];
                mel_mirror_partners(v, pz, lane);
                x256 = 2.0f * (MEL_RE(v[0]) - MEL_IM(v[0]));                 // 2 X[256] = 2 (Re Z[0] - Im Z[0])  (lane 0)
                if (l == 0) pw[4 * 256 + grp] = x256 * x256;
                mel_unpack(v, pz, tw512, l, xs);
            }
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const cplx q = csqr2(xs[k2]);
                pw[4 * (l + 16 * k2) + grp] = MEL_RE(q) + MEL_IM(q);          // the power spectrum times four, as the forward keeps it
            }
            wave_lds_sync();
            // ---- the mel bands of the four frames (the forward's projection), then dmel into LDS
            {
                const f32x4_t* pwq = reinterpret_cast<const f32x4_t*>(xch);
                f32x4_t acc_a = {0.0f, 0.0f, 0.0f, 0.0f}, acc_b = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const f32x4_t pa = pwq[sa + i], pb = pwq[sb + i];
                    acc_a = __builtin_elementwise_fma(pa, f32x4_t{wa[i], wa[i], wa[i], wa[i]}, acc_a);
                    acc_b = __builtin_elementwise_fma(pb, f32x4_t{wb[i], wb[i], wb[i], wb[i]}, acc_b);
                }
#pragma unroll 1
                for (int i = 8; i < na; ++i) acc_a += pwq[sa + i] * fb_w[lane * fb_stride + i];
#pragma unroll
                for (int f = 0; f < 4; ++f) acc_b[f] += mel_lane_xor1(acc_b[f]);
                if ((lane & 1) == 0)
#pragma unroll 1
                    for (int i = 16; i < nb; ++i) acc_b += pwq[sb + i] * fb_w[mbnd * fb_stride + i];
                f32x4_t da, db;
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const int tt = t0 + tl0 + f;
                    const float ga = tt < T ? gsrc[(int64_t)lane * T + tt] : 0.0f;
                    const float gb = tt < T ? gsrc[(int64_t)mbnd * T + tt] : 0.0f;
                    da[f] = ga * dcoef / __builtin_fmaf(acc_a[f], ls4, 1.0f);
                    db[f] = gb * dcoef / __builtin_fmaf(acc_b[f], ls4, 1.0f);
                }
                wave_lds_sync();                      // every lane has read the power spectra (dml lies behind them: no overlap, but keep the order)
                dml[lane] = da;
                if ((lane & 1) == 0) dml[mbnd] = db;
            }
            wave_lds_sync();
            // ---- dP per bin (at most two bands), H = dP X with the mirror-less bins doubled, conj H
            const float* dmf = reinterpret_cast<const float*>(dml);
            cplx hc[16];
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const int k = l + 16 * k2;
                const float dp = bwt[2 * k] * dmf[bband[2 * k] + grp] + bwt[2 * k + 1] * dmf[bband[2 * k + 1] + grp];
                const float c = (k2 == 0 && l == 0) ? dp : 0.5f * dp;       // H[0] = 2 dP X[0]; H[k] = dP X[k]; xs = 2 X
                hc[k2] = cplx{c * MEL_RE(xs[k2]), -(c * MEL_IM(xs[k2]))};
            }
            float h256;
            {
                h256 = (bwt[512] * dmf[bband[512] + grp] + bwt[513] * dmf[bband[513] + grp]) * x256;
            }
            // ---- inverse: conj(Zi) from conj H and its mirror (k = 0 pairs with H[256]), the 256-point DFT, conj -> (even, odd) samples
            {
                cplx pz[16];
                mel_mirror_partners(hc, pz, lane);
                if (l == 0) pz[0] = cplx{h256, 0.0f};
                mel_unpack(hc, pz, tw512, l, v);
            }
            wave_lds_sync();                          // dmel / the power spectra are read: the exchange tiles are free
            mel_fft256(v, xch + grp * MEL_XFRAME, tw256, l);
            if (t < T) {
                float* dst = dframes + ((int64_t)b * T + t) * MEL_NFFT;
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2) {
                    const int m = l + 16 * k2;        // samples 2 m, 2 m + 1 = (Re, -Im)
                    const cplx w2 = *reinterpret_cast<const cplx*>(wtab + 2 * m);
                    *reinterpret_cast<cplx*>(dst + 2 * m) = cplx{w2[0] * MEL_RE(v[k2]), -(w2[1] * MEL_IM(v[k2]))};
                }
            }
        }
    };
    if (interior) frames(std::true_type{});
    else frames(std::false_type{});
}

// Overlap-add + reflect fold: one thread per sample j of clip b, its contributions in a fixed order -- frame j / 256 (n = 256 + j mod 256),
// frame j / 256 + 1 (n = j mod 256), the left fold (padded index -j, 1 <= j <= 256: frame 0, n = 256 - j), the right fold (padded index
// 2 (S - 1) - j >= S: frame T - 1 only, where it reaches).
__global__ __launch_bounds__(256) void logmel_bwd_gather_kernel(const float* __restrict__ dframes, int S, int T, float* __restrict__ dwave) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= S) return;
    const float* d = dframes + (int64_t)b * T * MEL_NFFT;
    const int ta = j / MEL_HOP, r = j % MEL_HOP;          // ta <= (S - 1) / 256 <= T - 1
    float acc = d[(int64_t)ta * MEL_NFFT + MEL_HOP + r];
    if (ta + 1 < T) acc += d[(int64_t)(ta + 1) * MEL_NFFT + r];
    if (j >= 1 && j <= MEL_NFFT / 2) acc += d[MEL_NFFT / 2 - j];
    const int ir = 2 * (S - 1) - j;                       // >= S  <=>  j <= S - 2
    const int last0 = (T - 1) * MEL_HOP - MEL_NFFT / 2;   // first padded index of frame T - 1
    if (j <= S - 2 && ir - last0 < MEL_NFFT) acc += d[(int64_t)(T - 1) * MEL_NFFT + ir - last0];
    dwave[(int64_t)b * S + j] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Polyphase resampler (the front of maest_amd/mel_extractor.py: audio at any rate -> 16 kHz), torchaudio.functional.resample's
// sinc_interp_hann with the rates reduced by their gcd (orig -> new): output j = new q + p of a track is
//   y[j] = sum_k taps[p][k] xpad[orig q + k],   xpad = `width` zeros, x, `width + orig` zeros,
// and the host keeps only each phase's non-zero band (|t| < lowpass_filter_width): tap i of phase p multiplies x[orig q + first[p] + i - width]
// (zero outside the track).  One thread per output sample, the taps tap-major ([i][p]: a wave's consecutive phases read one run); fp32
// products summed by fma in tap order.
constexpr int RS_TRACK_FIELDS = 4;       // maest_resample's track table: input offset, input length, output offset, output length
constexpr int RS_BLOCK = 256;            // output samples per block
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(const float* __restrict__ in, int64_t total_in,
                                                           const int64_t* __restrict__ tracks, const int32_t* __restrict__ block_start,
                                                           int n_tracks, int orig, int nw, int width,
                                                           const float* __restrict__ taps, const int32_t* __restrict__ first, int n_taps,
                                                           float* __restrict__ out, int64_t total_out) {
    const int bid = blockIdx.x;
    int lo = 0, hi = n_tracks - 1;               // the last track whose first block is <= bid
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block_start[mid] <= bid) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* tr = tracks + RS_TRACK_FIELDS * lo;
    const int64_t off = tr[0], S = tr[1], o0 = tr[2], n_out = tr[3];
    const int64_t j = (int64_t)(bid - block_start[lo]) * RS_BLOCK + threadIdx.x;
    if (!(off >= 0 && S >= 1 && off + S <= total_in && o0 >= 0 && o0 + n_out <= total_out) || j < 0 || j >= n_out) return;
    const int64_t q = j / nw;
    const int p = (int)(j - q * nw);
    const float* x = in + off;
    const int64_t i0 = q * orig + first[p] - width;          // the input index of tap 0
    float acc = 0.0f;
    if (i0 >= 0 && i0 + n_taps <= S) {
        for (int i = 0; i < n_taps; ++i) acc = __builtin_fmaf(taps[(int64_t)i * nw + p], x[i0 + i], acc);
    } else {
        for (int i = 0; i < n_taps; ++i) {
            const int64_t k = i0 + i;
            const float v = k >= 0 && k < S ? x[k] : 0.0f;
            acc = __builtin_fmaf(taps[(int64_t)i * nw + p], v, acc);
        }
    }
    out[o0 + j] = acc;
}

}  // namespace maest

using namespace maest;

extern "C" int maest_logmel(const float* wave, int B, int S, const float* window, const float* twiddle,
                            const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                            float log_scale, float norm_mean, float norm_2std, float* out, void* stream) {
    MAEST_REQUIRE(wave && window && twiddle && fb_start && fb_len && fb_w && out, "maest_logmel: null pointer");
    MAEST_REQUIRE(B > 0 && S > MEL_NFFT / 2, "maest_logmel: bad shape B=%d S=%d (reflect padding needs S > 256)", B, S);
    MAEST_REQUIRE(fb_stride > 0, "maest_logmel: bad fb_stride");
    const int T = 1 + S / MEL_HOP;
    const int smem_bytes = (512 + 512 + 512 + MEL_BANDS * MEL_OUT_LD) * 4 + 4 * 4 * MEL_XFRAME;
    dim3 grid((T + MEL_FRAMES_PER_BLOCK - 1) / MEL_FRAMES_PER_BLOCK, B);
    static DeviceOnce once;                       // 70 KiB of dynamic LDS: above the 64 KiB a kernel gets without the attribute
    ensure_dynamic_lds(once, &logmel_kernel<MelEpiBandMajor>, smem_bytes);
    hipLaunchKernelGGL(logmel_kernel<MelEpiBandMajor>, grid, dim3(256), smem_bytes, (hipStream_t)stream, wave, S, T, window, twiddle,
                       fb_start, fb_len, fb_w, fb_stride, log_scale, norm_mean, norm_2std, MelEpiBandMajor{out});
    return check_launch("maest_logmel");
}

extern "C" int maest_logmel_bwd(const float* wave, const float* grad_out, int B, int S, const float* window, const float* twiddle,
                                const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                                const int32_t* bin_band, const float* bin_w, float log_scale, float norm_mean, float norm_2std,
                                float* work, int64_t work_elems, float* dwave, void* stream) {
    (void)norm_mean;                              // the mean shifts the output, not its gradient
    MAEST_REQUIRE(wave && grad_out && window && twiddle && fb_start && fb_len && fb_w && bin_band && bin_w && work && dwave,
                  "maest_logmel_bwd: null pointer");
    MAEST_REQUIRE(B > 0 && S > MEL_NFFT / 2, "maest_logmel_bwd: bad shape B=%d S=%d (reflect padding needs S > 256)", B, S);
    MAEST_REQUIRE(fb_stride > 0, "maest_logmel_bwd: bad fb_stride");
    const int T = 1 + S / MEL_HOP;
    MAEST_REQUIRE(work_elems >= (int64_t)B * T * MEL_NFFT, "maest_logmel_bwd: workspace of %lld floats, needs B * T * 512 = %lld",
                  (long long)work_elems, (long long)B * T * MEL_NFFT);
    const int smem_bytes = (512 + 512 + 512) * 4 + 2 * 2 * 260 * 4 + 4 * 4 * MEL_XFRAME;
    hipLaunchKernelGGL(logmel_bwd_frames_kernel, dim3((T + MEL_FRAMES_PER_BLOCK - 1) / MEL_FRAMES_PER_BLOCK, B), dim3(256), smem_bytes,
                       (hipStream_t)stream, wave, S, T, window, twiddle, fb_start, fb_len, fb_w, fb_stride, bin_band, bin_w, grad_out,
                       log_scale, norm_2std, work);
    int rc = check_launch("maest_logmel_bwd (frames)");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(logmel_bwd_gather_kernel, dim3((S + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, work, S, T, dwave);
    return check_launch("maest_logmel_bwd (gather)");
}

extern "C" int maest_logmel_rows_f16(const float* wave, int64_t total_in, const int64_t* tracks, const int32_t* block_start, int n_tracks,
                                     int n_blocks, const float* window, const float* twiddle, const int32_t* fb_start, const int32_t* fb_len,
                                     const float* fb_w, int fb_stride, float log_scale, void* rows, int64_t total_rows, void* stream) {
    MAEST_REQUIRE(wave && tracks && block_start && window && twiddle && fb_start && fb_len && fb_w && rows,
                  "maest_logmel_rows_f16: null pointer");
    MAEST_REQUIRE(n_tracks > 0 && n_blocks > 0, "maest_logmel_rows_f16: bad shape n_tracks=%d n_blocks=%d", n_tracks, n_blocks);
    MAEST_REQUIRE(total_in > MEL_NFFT / 2, "maest_logmel_rows_f16: bad shape total_in=%lld (reflect padding needs S > 256)",
                  (long long)total_in);
    MAEST_REQUIRE(total_rows > 0, "maest_logmel_rows_f16: bad shape total_rows=%lld", (long long)total_rows);
    MAEST_REQUIRE(fb_stride > 0, "maest_logmel_rows_f16: bad fb_stride");
    MAEST_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "maest_logmel_rows_f16: rows must be 16-byte aligned");
    const int smem_bytes = (512 + 512 + 512 + MEL_BANDS * MEL_OUT_LD) * 4 + 4 * 4 * MEL_XFRAME;
    static DeviceOnce once;
    ensure_dynamic_lds(once, &logmel_kernel<MelEpiRowsF16>, smem_bytes);
    MelEpiRowsF16 epi{tracks, block_start, n_tracks, total_in, total_rows, static_cast<_Float16*>(rows)};
    // log10(1 + s mel): the forward's epilogue with mean 0 and 2 std 1
    hipLaunchKernelGGL(logmel_kernel<MelEpiRowsF16>, dim3(n_blocks), dim3(256), smem_bytes, (hipStream_t)stream, wave, 0, 0, window,
                       twiddle, fb_start, fb_len, fb_w, fb_stride, log_scale, 0.0f, 1.0f, epi);
    return check_launch("maest_logmel_rows_f16");
}

extern "C" int maest_resample(const float* in, int64_t total_in, const int64_t* tracks, const int32_t* block_start, int n_tracks,
                              int n_blocks, int orig, int new_rate, int width, const float* taps, const int32_t* first, int n_taps,
                              float* out, int64_t total_out, void* stream) {
    MAEST_REQUIRE(in && tracks && block_start && taps && first && out, "maest_resample: null pointer");
    MAEST_REQUIRE(n_tracks > 0 && n_blocks > 0 && total_in > 0 && total_out > 0,
                  "maest_resample: bad shape n_tracks=%d n_blocks=%d total_in=%lld total_out=%lld", n_tracks, n_blocks,
                  (long long)total_in, (long long)total_out);
    MAEST_REQUIRE(orig > 0 && new_rate > 0 && width >= 0 && n_taps > 0 && n_taps <= 2 * width + orig,
                  "maest_resample: bad filter orig=%d new=%d width=%d n_taps=%d", orig, new_rate, width, n_taps);
    hipLaunchKernelGGL(resample_kernel, dim3(n_blocks), dim3(RS_BLOCK), 0, (hipStream_t)stream, in, total_in, tracks, block_start,
                       n_tracks, orig, new_rate, width, taps, first, n_taps, out, total_out);
    return check_launch("maest_resample");
}
