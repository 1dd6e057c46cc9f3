// Second log-mel parameterisation: AugmentMelSTFT (reference: models/preprocess.py:17-128 -- 32 kHz, pre-emphasis
// [-0.97, 1] :82-84, torch.stft(n_fft = 1024, hop = 320, win = 800 non-periodic Hann, center = True) :85-94, power
// spectrum :95, 128 kaldi mel banks with fmin / fmax jitter :96-121, log(x + 1e-5) :123, (x + 4.5) / 5 :129).
// Named in north_star; dead code in the reference's MAEST path, so this is the same fused
// design as mel.hip instantiated for the other constants rather than a tuned kernel: one pass over HBM, a
// workgroup owns 32 consecutive frames of one clip, each wave transforms 8 of them in LDS with a 1024-point
// radix-4 complex FFT (5 stages, 4 butterflies per lane per stage; the input is real, bins 0..512 are used), the
// filterbank comes in band-sparse form from the host (it changes per call under fmin / fmax augmentation).
#include "common.h"

namespace maest {

constexpr int M2_NFFT = 1024;
constexpr int M2_HOP = 320;
constexpr int M2_NBINS = 513;
constexpr int M2_FPB = 32;            // frames per block
constexpr int M2_OUT_LD = M2_FPB + 1;
constexpr int M2_MAXBANDS = 128;

struct cplx2 {
    float re, im;
};
__device__ __forceinline__ cplx2 c2add(cplx2 a, cplx2 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx2 c2sub(cplx2 a, cplx2 b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx2 c2mul(cplx2 a, cplx2 b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx2 c2mul_neg_i(cplx2 a) { return {a.im, -a.re}; }
__device__ __forceinline__ int rev4_1024(int k) {   // reverse the five base-4 digits of k
    return ((k & 3) << 8) | (((k >> 2) & 3) << 6) | (((k >> 4) & 3) << 4) | (((k >> 6) & 3) << 2) | ((k >> 8) & 3);
}

// Frame t of one clip into a wave's z[1024]: pre-emphasis + framing (center = True, reflect padding of 512 on the Sy = S - 1 pre-emphasised
// samples) + window.
__device__ __forceinline__ void m2_load_frame(cplx2* z, const float* __restrict__ wsrc, const float* __restrict__ window, int t, int Sy,
                                              float pre0, float pre1, int lane) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int p = lane + 64 * j;
        int i = t * M2_HOP + p - M2_NFFT / 2;
        if (i < 0) i = -i;
        if (i >= Sy) i = 2 * (Sy - 1) - i;
        const float y = pre0 * wsrc[i] + pre1 * wsrc[i + 1];
        z[p] = {y * window[p], 0.0f};
    }
}

// The 1024-point complex FFT of a wave's z[1024] in LDS, in place: radix-4 DIF, five stages, four butterflies per lane per stage;
// X[k] is left at z[rev4_1024(k)].  tw: [1024][2] = exp(-2 pi i k / 1024) in LDS.  All four waves of the block call it together (block
// barriers between the stages); the caller's writes to z are behind a barrier on entry, and the result is behind one on return.
__device__ __forceinline__ void m2_fft1024(cplx2* z, const float* tw, int lane) {
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int L = M2_NFFT >> (2 * st);
        const int q = L >> 2;
        cplx2 y[4][4];
        int base[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = lane + 64 * u;
            const int blk = j / q, pos = j - blk * q;
            base[u] = blk * L + pos;
            const cplx2 a0 = z[base[u]], a1 = z[base[u] + q], a2 = z[base[u] + 2 * q], a3 = z[base[u] + 3 * q];
            const cplx2 b0 = c2add(a0, a2), b1 = c2sub(a0, a2), b2 = c2add(a1, a3), b3 = c2mul_neg_i(c2sub(a1, a3));
            const int tstep = (M2_NFFT / L) * pos;
            const cplx2 w1 = {tw[2 * tstep], tw[2 * tstep + 1]};
            const cplx2 w2 = {tw[4 * tstep], tw[4 * tstep + 1]};
            const cplx2 w3 = {tw[6 * tstep], tw[6 * tstep + 1]};
            y[u][0] = c2add(b0, b2);
            y[u][1] = c2mul(c2add(b1, b3), w1);
            y[u][2] = c2mul(c2sub(b0, b2), w2);
            y[u][3] = c2mul(c2sub(b1, b3), w3);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            z[base[u]] = y[u][0]; z[base[u] + q] = y[u][1]; z[base[u] + 2 * q] = y[u][2]; z[base[u] + 3 * q] = y[u][3];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void augment_mel_kernel(const float* __restrict__ wave_in, int S, int T,
                                                          const float* __restrict__ window,     // [1024], zero padded
                                                          const float* __restrict__ twiddle,    // [1024][2]
                                                          const int32_t* __restrict__ fb_start,
                                                          const int32_t* __restrict__ fb_len,
                                                          const float* __restrict__ fb_w, int fb_stride, int n_mels,
                                                          float pre0, float pre1, float log_eps, float norm_add,
                                                          float norm_div, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* tw = reinterpret_cast<float*>(smem);                       // [2048]
    float* otile = tw + 2048;                                         // [128][33]
    cplx2* zall = reinterpret_cast<cplx2*>(otile + M2_MAXBANDS * M2_OUT_LD);
    cplx2* z = zall + wv * M2_NFFT;                                   // per wave [1024]
    float* pw = reinterpret_cast<float*>(zall + 4 * M2_NFFT) + wv * 516;

    for (int i = threadIdx.x; i < 2048; i += 256) tw[i] = twiddle[i];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * M2_FPB;
    const float* wsrc = wave_in + (int64_t)b * S;
    const int Sy = S - 1;                                             // length after the 2-tap pre-emphasis
    __syncthreads();

    for (int fi = 0; fi < M2_FPB / 4; ++fi) {
        const int tl = wv * (M2_FPB / 4) + fi;
        const int t = t0 + tl;
        m2_load_frame(z, wsrc, window, t < T ? t : T - 1, Sy, pre0, pre1, lane);
        __syncthreads();
        // ---- 1024-point complex FFT, radix-4 DIF
        m2_fft1024(z, tw, lane);
        // ---- power spectrum of bins 0 .. 512
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = lane + 64 * j;
            if (k < M2_NBINS) {
                const cplx2 x = z[rev4_1024(k)];
                pw[k] = x.re * x.re + x.im * x.im;
            }
        }
        __syncthreads();
        // ---- mel projection, log, affine normalisation
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = lane + 64 * j;
            if (m < n_mels) {
                const int s0 = fb_start[m], n = fb_len[m];
                float acc = 0.0f;
                for (int i = 0; i < n; ++i) acc += pw[s0 + i] * fb_w[m * fb_stride + i];
                otile[m * M2_OUT_LD + tl] = (logf(acc + log_eps) + norm_add) / norm_div;
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n_mels * M2_FPB; i += 256) {
        const int m = i / M2_FPB, tl = i - m * M2_FPB;
        if (t0 + tl < T) out[((int64_t)b * n_mels + m) * T + t0 + tl] = otile[m * M2_OUT_LD + tl];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Backward of augment_mel_kernel: dwave from g = dL/dout.  Per frame t (fp32 throughout; X = the frame's spectrum, recomputed here rather
// than saved: it is larger than the waveform; acc[m] = the mel bands of the frame):
//   dacc[m] = g[m] / (norm_div (acc[m] + log_eps))
//   dP[k]   = sum_m fb[m, k] dacc[m]                                            (a bin lies in <= 2 bands: per-bin table, no scatter)
//   dz[p]   = sum_{k=0}^{512} 2 dP[k] Re(X[k] exp(+2 pi i k p / 1024))          = the real inverse DFT of the Hermitian H with
//             H[k] = dP[k] X[k] (k = 1 .. 511), H[1024 - k] = conj H[k], H[0] = 2 dP[0] X[0], H[512] = 2 dP[512] X[512]  (no mirror)
//             -- the forward transform of conj(H) is conj(dz), so m2_fft1024 serves both directions
//   dframe[p] = win[p] dz[p]
// then overlap-add at hop 320 with both reflect folds folded back onto y, and the adjoint of the pre-emphasis.  Two kernels, the design of
// maest_logmel_bwd: augment_mel_bwd_frames_kernel writes dframe of every frame to an fp32 scratch [B, T, 1024];
// augment_mel_bwd_gather_kernel gives each sample ONE thread that adds its contributions in a fixed order -- deterministic, no atomics.

constexpr int M2_BINLD = 516;         // LDS pitch of the per-bin tables and of a wave's power spectrum (513 bins)

// The forward's block shape: 32 consecutive frames of one clip, 8 per wave, one at a time through the wave's z[1024].
__global__ __launch_bounds__(256) void augment_mel_bwd_frames_kernel(const float* __restrict__ wave_in, int S, int T,
                                                                     const float* __restrict__ window,
                                                                     const float* __restrict__ twiddle,
                                                                     const int32_t* __restrict__ fb_start,
                                                                     const int32_t* __restrict__ fb_len,
                                                                     const float* __restrict__ fb_w, int fb_stride, int n_mels,
                                                                     const int32_t* __restrict__ bin_band,   // [513][2]
                                                                     const float* __restrict__ bin_w,        // [513][2]
                                                                     const float* __restrict__ grad_out,     // [B, n_mels, T]
                                                                     float pre0, float pre1, float log_eps, float norm_div,
                                                                     float* __restrict__ dframes) {          // [B, T, 1024]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* tw = reinterpret_cast<float*>(smem);                       // [2048]
    int32_t* bband = reinterpret_cast<int32_t*>(tw + 2048);           // [513][2] the bands of each bin (times the tile's pitch)
    float* bwt = tw + 2048 + 2 * M2_BINLD;                            // [513][2] their weights
    float* gtile = bwt + 2 * M2_BINLD;                                // [128][33] g of the block's frames, then dacc in place
    cplx2* zall = reinterpret_cast<cplx2*>(gtile + M2_MAXBANDS * M2_OUT_LD);
    cplx2* z = zall + wv * M2_NFFT;                                   // per wave [1024]
    float* pw = reinterpret_cast<float*>(zall + 4 * M2_NFFT) + wv * M2_BINLD;

    const int b = blockIdx.y;
    const int t0 = blockIdx.x * M2_FPB;
    const float* wsrc = wave_in + (int64_t)b * S;
    const int Sy = S - 1;
    for (int i = threadIdx.x; i < 2048; i += 256) tw[i] = twiddle[i];
    for (int i = threadIdx.x; i < 2 * M2_NBINS; i += 256) {
        const int m = bin_band[i];                                    // (clamped: a bad table reads a wrong band, never outside the tile)
        bband[i] = (m < 0 ? 0 : m >= n_mels ? n_mels - 1 : m) * M2_OUT_LD;
        bwt[i] = bin_w[i];
    }
    for (int i = threadIdx.x; i < n_mels * M2_FPB; i += 256) {        // frames >= T: zero gradient, transformed but not stored
        const int m = i / M2_FPB, tl = i - m * M2_FPB;
        gtile[m * M2_OUT_LD + tl] = t0 + tl < T ? grad_out[((int64_t)b * n_mels + m) * T + t0 + tl] : 0.0f;
    }
    __syncthreads();

    for (int fi = 0; fi < M2_FPB / 4; ++fi) {
        const int tl = wv * (M2_FPB / 4) + fi;
        const int t = t0 + tl;
        // ---- the forward, recomputed: frame, spectrum (kept in registers: bin k = lane + 64 j), power spectrum
        m2_load_frame(z, wsrc, window, t < T ? t : T - 1, Sy, pre0, pre1, lane);
        __syncthreads();
        m2_fft1024(z, tw, lane);
        cplx2 x[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = lane + 64 * j;
            x[j] = {0.0f, 0.0f};
            if (k < M2_NBINS) {
                x[j] = z[rev4_1024(k)];
                pw[k] = x[j].re * x[j].re + x[j].im * x[j].im;
            }
        }
        __syncthreads();
        // ---- the mel bands (the forward's projection), dacc over g in the tile
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = lane + 64 * j;
            if (m < n_mels) {
                const int s0 = fb_start[m], n = fb_len[m];
                float acc = 0.0f;
                for (int i = 0; i < n; ++i) acc += pw[s0 + i] * fb_w[m * fb_stride + i];
                gtile[m * M2_OUT_LD + tl] = gtile[m * M2_OUT_LD + tl] / (norm_div * (acc + log_eps));
            }
        }
        __syncthreads();
        // ---- dP per bin (at most two bands), conj H over all 1024 bins (every lane has its X in registers: z is free)
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = lane + 64 * j;
            if (k < M2_NBINS) {
                const float dp = bwt[2 * k] * gtile[bband[2 * k] + tl] + bwt[2 * k + 1] * gtile[bband[2 * k + 1] + tl];
                const bool mirrored = k >= 1 && k < M2_NFFT / 2;
                const float c = mirrored ? dp : 2.0f * dp;
                const float hr = c * x[j].re, hi = c * x[j].im;
                z[k] = {hr, -hi};
                if (mirrored) z[M2_NFFT - k] = {hr, hi};
            }
        }
        __syncthreads();
        // ---- inverse transform (the forward one on conj H), window, the frame's gradient to the scratch
        m2_fft1024(z, tw, lane);
        if (t < T) {
            float* dst = dframes + ((int64_t)b * T + t) * M2_NFFT;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int p = lane + 64 * j;
                dst[p] = window[p] * z[rev4_1024(p)].re;
            }
        }
        __syncthreads();       // z is refilled by the next frame
    }
}

// The sum over the frames t (ascending) whose 1024-sample span holds padded position u of y (u = 320 t + p - 512, 0 <= p < 1024): at most four.
__device__ __forceinline__ float m2_frames_at(const float* __restrict__ d, int T, int u) {
    const int q = u + M2_NFFT / 2;
    if (q < 0) return 0.0f;
    const int tlo = q < M2_NFFT ? 0 : (q - M2_NFFT) / M2_HOP + 1;     // the first t with q - 320 t <= 1023
    int thi = q / M2_HOP;
    if (thi > T - 1) thi = T - 1;
    float acc = 0.0f;
    for (int t = tlo; t <= thi; ++t) acc += d[(int64_t)t * M2_NFFT + q - t * M2_HOP];
    return acc;
}
// dL/dy[i] of one clip: the frames at i itself, then the left fold (padded index -i, 1 <= i <= 512), then the right fold (padded index
// 2 (Sy - 1) - i >= Sy, up to Sy + 511); 0 outside 0 .. Sy - 1.
__device__ __forceinline__ float m2_dy(const float* __restrict__ d, int Sy, int T, int i) {
    if (i < 0 || i >= Sy) return 0.0f;
    float acc = m2_frames_at(d, T, i);
    if (i >= 1 && i <= M2_NFFT / 2) acc += m2_frames_at(d, T, -i);
    const int back = Sy - 1 - i;
    if (back >= 1 && back <= M2_NFFT / 2) acc += m2_frames_at(d, T, Sy - 1 + back);
    return acc;
}

// Overlap-add + reflect folds + the adjoint of the pre-emphasis y[i] = pre0 x[i] + pre1 x[i + 1]: dwave[n] = pre0 dy[n] + pre1 dy[n - 1].
// One thread sums dy of one sample; its neighbour's comes through LDS (thread 0 also sums the one in front of the block).
__global__ __launch_bounds__(256) void augment_mel_bwd_gather_kernel(const float* __restrict__ dframes, int S, int T, float pre0, float pre1,
                                                                     float* __restrict__ dwave) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dy = reinterpret_cast<float*>(smem);                       // [257]: dy[n0 - 1 .. n0 + 255]
    const int n0 = blockIdx.x * 256, b = blockIdx.y;
    const int n = n0 + threadIdx.x;
    const float* d = dframes + (int64_t)b * T * M2_NFFT;
    dy[threadIdx.x + 1] = m2_dy(d, S - 1, T, n);
    if (threadIdx.x == 0) dy[0] = m2_dy(d, S - 1, T, n0 - 1);
    __syncthreads();
    if (n < S) dwave[(int64_t)b * S + n] = pre0 * dy[threadIdx.x + 1] + pre1 * dy[threadIdx.x];
}

}  // namespace maest

using namespace maest;

extern "C" int maest_augment_mel(const float* wave, int B, int S, const float* window, const float* twiddle,
                                 const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                                 int n_mels, float pre0, float pre1, float log_eps, float norm_add, float norm_div,
                                 float* out, void* stream) {
    MAEST_REQUIRE(wave && window && twiddle && fb_start && fb_len && fb_w && out, "maest_augment_mel: null pointer");
    MAEST_REQUIRE(B > 0 && S > M2_NFFT / 2 + 1, "maest_augment_mel: bad shape B=%d S=%d (reflect padding needs S > 513)", B, S);
    MAEST_REQUIRE(n_mels > 0 && n_mels <= M2_MAXBANDS && fb_stride > 0, "maest_augment_mel: bad filterbank n_mels=%d", n_mels);
    const int T = 1 + (S - 1) / M2_HOP;
    const int smem_bytes = (2048 + M2_MAXBANDS * M2_OUT_LD) * 4 + 4 * M2_NFFT * 8 + 4 * 516 * 4;
    static DeviceOnce once;
    ensure_dynamic_lds(once, &augment_mel_kernel, smem_bytes);
    dim3 grid((T + M2_FPB - 1) / M2_FPB, B);
    hipLaunchKernelGGL(augment_mel_kernel, grid, dim3(256), smem_bytes, (hipStream_t)stream, wave, S, T, window, twiddle,
                       fb_start, fb_len, fb_w, fb_stride, n_mels, pre0, pre1, log_eps, norm_add, norm_div, out);
    return check_launch("maest_augment_mel");
}

extern "C" int maest_augment_mel_bwd(const float* wave, const float* grad_out, int B, int S, const float* window, const float* twiddle,
                                     const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride, int n_mels,
                                     const int32_t* bin_band, const float* bin_w, float pre0, float pre1, float log_eps, float norm_div,
                                     float* work, int64_t work_elems, float* dwave, void* stream) {
    MAEST_REQUIRE(wave && grad_out && window && twiddle && fb_start && fb_len && fb_w && bin_band && bin_w && work && dwave,
                  "maest_augment_mel_bwd: null pointer");
    MAEST_REQUIRE(B > 0 && S > M2_NFFT / 2 + 1, "maest_augment_mel_bwd: bad shape B=%d S=%d (reflect padding needs S > 513)", B, S);
    MAEST_REQUIRE(n_mels > 0 && n_mels <= M2_MAXBANDS && fb_stride > 0, "maest_augment_mel_bwd: bad filterbank n_mels=%d fb_stride=%d",
                  n_mels, fb_stride);
    const int T = 1 + (S - 1) / M2_HOP;
    MAEST_REQUIRE(work_elems >= (int64_t)B * T * M2_NFFT, "maest_augment_mel_bwd: workspace of %lld floats, needs B * T * 1024 = %lld",
                  (long long)work_elems, (long long)B * T * M2_NFFT);
    const int smem_bytes = (2048 + 4 * M2_BINLD + M2_MAXBANDS * M2_OUT_LD) * 4 + 4 * M2_NFFT * 8 + 4 * M2_BINLD * 4;
    static DeviceOnce once;                       // 73 KiB of dynamic LDS
    ensure_dynamic_lds(once, &augment_mel_bwd_frames_kernel, smem_bytes);
    hipLaunchKernelGGL(augment_mel_bwd_frames_kernel, dim3((T + M2_FPB - 1) / M2_FPB, B), dim3(256), smem_bytes, (hipStream_t)stream, wave,
                       S, T, window, twiddle, fb_start, fb_len, fb_w, fb_stride, n_mels, bin_band, bin_w, grad_out, pre0, pre1, log_eps,
                       norm_div, work);
    int rc = check_launch("maest_augment_mel_bwd (frames)");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(augment_mel_bwd_gather_kernel, dim3((S + 255) / 256, B), dim3(256), 257 * 4, (hipStream_t)stream, work, S, T, pre0,
                       pre1, dwave);
    return check_launch("maest_augment_mel_bwd (gather)");
}
