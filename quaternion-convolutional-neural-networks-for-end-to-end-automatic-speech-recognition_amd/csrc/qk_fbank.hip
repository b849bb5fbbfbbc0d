// Acoustic front end: waveforms -> the model's (B, 4, nfilt [+ 1], T) channels_first quaternion input.  The recipe is
// python_speech_features' logfbank + delta (semantics and limits: include/qk.h, "Acoustic front end"); all arithmetic is fp32.
//
//   k_fbank_static  one 256-thread workgroup per (tile of up to 16 frames, utterance).  The tile's sample span is staged once in LDS
//                   (pre-emphasis applied there; consecutive frames overlap), then each wave takes one frame at a time: the real
//                   nfft-point FFT as an nfft/2-point complex radix-2 Stockham FFT in LDS (even samples real, odd imaginary) plus the
//                   real-input post-twiddle, |X|^2 / nfft, the triangular mel filters (one lane per filter, bins [b_j, b_j+2)), the
//                   frame energy, the eps floor and the log.  Twiddles and the window are formed per workgroup in double.
//                   -> fp32 static rows (B, F, T) in the workspace, and the frame count of each utterance.
//   k_fbank_delta   one wave per (row, 64-frame tile, utterance): the static row with a halo of 3N frames, then delta, delta^2, delta^3
//                   in LDS, each clamped to the utterance's own frames [0, n_b); stage s is evaluated on the tile widened by (3 - s) N.
//                   Writes the four planes in the output dtype (or fp32 to the workspace when normalising) and zeros for t >= n_b.
//   k_fbank_norm    one wave per (utterance, plane, row): mean and biased variance over the valid frames (two passes), then
//                   (x - mean) / sqrt(var + 1e-8) in the output dtype; padding stays 0.
#include "qk_common.h"

namespace qk {
namespace {

constexpr int FB_THREADS = 256;
constexpr int FB_WAVES = FB_THREADS / 64;
constexpr int FB_TILE = 16;             // frames per workgroup of k_fbank_static
constexpr int FB_SPAN_MAX = 4096;       // staged samples per workgroup (the tile shrinks for long frame steps): LDS stays <= 64 KiB
constexpr int DL_TILE = 64;             // frames per wave of k_fbank_delta
constexpr int DL_ROWS = FB_THREADS / 64;
constexpr int kMaxDelta = 4;
constexpr int DL_WIDTH = DL_TILE + 6 * kMaxDelta;
constexpr float kLogEps = -36.04365338911715f;            // log(2.220446049250313e-16): numpy's float64 eps, the floor of exact zeros

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ int frames_of(int n, int L, int S) { return n <= L ? 1 : 1 + (n - L + S - 1) / S; }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__device__ __forceinline__ float to_sample(float v) { return v; }
__device__ __forceinline__ float to_sample(int16_t v) { return (float)v; }

// LDS of k_fbank_static, in floats: twiddles W_N^k (k < N/2, complex), window (L), span, per wave two buffers of N/2 complex
__host__ __device__ inline int fb_off_window(const FbankGeom &g) { return g.nfft; }
__host__ __device__ inline int fb_off_span(const FbankGeom &g) { return g.nfft + g.L; }
__host__ __device__ inline int fb_off_bufs(const FbankGeom &g) { return (fb_off_span(g) + g.span + 3) & ~3; }
__host__ __device__ inline size_t fb_lds_bytes(const FbankGeom &g) { return 4 * ((size_t)fb_off_bufs(g) + (size_t)FB_WAVES * 2 * g.nfft); }

template <typename Tin>
__global__ void __launch_bounds__(FB_THREADS)
k_fbank_static(const Tin *__restrict__ wave, const int *__restrict__ lengths, FbankGeom g, float *__restrict__ stat,
               int *__restrict__ frame_lengths)
{
    extern __shared__ float smem[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = min(max(lengths[b], 0), g.n_max);
    const int nf = frames_of(n, g.L, g.S);
    if (blockIdx.x == 0 && tid == 0) frame_lengths[b] = nf;
    const int t0 = blockIdx.x * g.tile;
    if (t0 >= nf) return;                                             // workgroup-uniform
    const int nt = min(g.tile, nf - t0);
    const int N = g.nfft, M = N >> 1;
    float2 *tw = reinterpret_cast<float2 *>(smem);
    float *win = smem + fb_off_window(g);
    float *sp = smem + fb_off_span(g);
    float2 *bufs = reinterpret_cast<float2 *>(smem + fb_off_bufs(g));

    for (int k = tid; k < M; k += FB_THREADS) {
        double s, c;
        sincospi(2.0 * k / N, &s, &c);
        tw[k] = make_float2((float)c, (float)-s);                     // e^{-2 pi i k / N}
    }
    for (int m = tid; m < g.L; m += FB_THREADS)
        win[m] = (g.window == QK_WINDOW_HAMMING && g.L > 1) ? (float)(0.54 - 0.46 * cos(2.0 * 3.141592653589793 * m / (g.L - 1))) : 1.f;
    const Tin *x = wave + (long long)b * g.n_max;
    const long long s0 = (long long)t0 * g.S;
    for (int u = tid; u < g.span; u += FB_THREADS) {
        const long long i = s0 + u;
        float v = 0.f;
        if (i < n) v = i == 0 ? to_sample(x[0]) : fmaf(-g.preemph, to_sample(x[i - 1]), to_sample(x[i]));
        sp[u] = v;
    }
    __syncthreads();

    const int hm = M >> 1;
    float2 *A = bufs + wid * 2 * M, *Bf = A + M;
    for (int f0 = 0; f0 < nt; f0 += FB_WAVES) {
        const int f = f0 + wid;
        const bool on = f < nt;                                       // the barriers below stay workgroup-uniform
        const float *fr = sp + f * g.S;
        // stage 0 (Ns = 1), fused with the frame load: z[m] = x[2m] + i x[2m+1], x zero beyond the frame length
        if (on) {
            for (int j = lane; j < hm; j += 64) {
                float2 a, c;
                const int q0 = 2 * j, q1 = 2 * (j + hm);
                a.x = q0 < g.L ? fr[q0] * win[q0] : 0.f;
                a.y = q0 + 1 < g.L ? fr[q0 + 1] * win[q0 + 1] : 0.f;
                c.x = q1 < g.L ? fr[q1] * win[q1] : 0.f;
                c.y = q1 + 1 < g.L ? fr[q1 + 1] * win[q1 + 1] : 0.f;
                A[2 * j] = make_float2(a.x + c.x, a.y + c.y);
                A[2 * j + 1] = make_float2(a.x - c.x, a.y - c.y);
            }
        }
        __syncthreads();
        float2 *src = A, *dst = Bf;
        for (int Ns = 2; Ns < M; Ns <<= 1) {
            if (on) {
                const int tws = M / Ns;
                for (int j = lane; j < hm; j += 64) {
                    const int k = j & (Ns - 1);
                    const float2 a = src[j], c = cmul(src[j + hm], tw[k * tws]);
                    const int o = 2 * (j - k) + k;
                    dst[o] = make_float2(a.x + c.x, a.y + c.y);
                    dst[o + Ns] = make_float2(a.x - c.x, a.y - c.y);
                }
            }
            __syncthreads();
            float2 *t = src; src = dst; dst = t;
        }
        // src = Z (natural order).  Real-input post-twiddle: X[k] = E + W_N^k O, E = (Z[k] + Z*[M-k]) / 2, O = -i (Z[k] - Z*[M-k]) / 2
        float *P = reinterpret_cast<float *>(dst);
        if (on) {
            const float inv_n = 1.f / (float)N;
            for (int k = lane; k <= M; k += 64) {
                const float2 zk = src[k & (M - 1)], zc = src[(M - k) & (M - 1)];
                const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
                const float2 o = make_float2(0.5f * (zk.y + zc.y), -0.5f * (zk.x - zc.x));
                const float2 w = k < M ? tw[k] : make_float2(-1.f, 0.f);
                const float2 wo = cmul(w, o);
                const float re = e.x + wo.x, im = e.y + wo.y;
                P[k] = (re * re + im * im) * inv_n;
            }
        }
        __syncthreads();
        if (on) {
            const int t = t0 + f;
            float *row = stat + (long long)b * g.F * g.T + t;
            for (int j = lane; j < g.nfilt; j += 64) {
                const int b0 = g.bins[j], b1 = g.bins[j + 1], b2 = g.bins[j + 2];
                float acc = 0.f;
                for (int i = b0; i < b1; ++i) acc += ((float)(i - b0) / (float)(b1 - b0)) * P[i];
                for (int i = b1; i < b2; ++i) acc += ((float)(b2 - i) / (float)(b2 - b1)) * P[i];
                row[(long long)j * g.T] = acc == 0.f ? kLogEps : logf(acc);
            }
            if (g.F > g.nfilt) {
                float e = 0.f;
                for (int k = lane; k <= M; k += 64) e += P[k];
                e = wave_sum(e);
                if (lane == 0) row[(long long)g.nfilt * g.T] = e == 0.f ? kLogEps : logf(e);
            }
        }
        __syncthreads();
    }
}

// d[t] = sum_{k=1..N} k (src[clamp(t + k)] - src[clamp(t - k)]) / (2 sum k^2), t and the clamp in utterance frames, src indexed from `base`
__device__ __forceinline__ float delta_at(const float *src, int t, int base, int nf, int N, float denom)
{
    float acc = 0.f;
    for (int k = 1; k <= N; ++k) acc += (float)k * (src[min(t + k, nf - 1) - base] - src[max(t - k, 0) - base]);
    return acc / denom;
}

template <typename To>
__global__ void __launch_bounds__(FB_THREADS)
k_fbank_delta(const float *__restrict__ stat, const int *__restrict__ frame_lengths, int F, int T, int N, To *__restrict__ out)
{
    __shared__ float lds[DL_ROWS][3][DL_WIDTH];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int b = blockIdx.z, f = blockIdx.y * DL_ROWS + wid, t0 = blockIdx.x * DL_TILE;
    const bool on = f < F;
    const int nf = frame_lengths[b];
    const int base = t0 - 3 * N, W0 = DL_TILE + 6 * N;
    const float denom = (float)(N * (N + 1) * (2 * N + 1) / 3);     // 2 sum_{k=1..N} k^2
    float *s = lds[wid][0], *d1 = lds[wid][1], *d2 = lds[wid][2];
    const float *row = stat + ((long long)b * F + (on ? f : 0)) * T;
    for (int u = lane; u < W0; u += 64) {
        const int t = base + u;
        s[u] = (on && t >= 0 && t < nf) ? row[t] : 0.f;
    }
    __syncthreads();
    for (int u = N + lane; u < W0 - N; u += 64) {
        const int t = base + u;
        if (t >= 0 && t < nf) d1[u] = delta_at(s, t, base, nf, N, denom);
    }
    __syncthreads();
    for (int u = 2 * N + lane; u < W0 - 2 * N; u += 64) {
        const int t = base + u;
        if (t >= 0 && t < nf) d2[u] = delta_at(d1, t, base, nf, N, denom);
    }
    __syncthreads();
    const int t = t0 + lane;
    if (!on || t >= T) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t < nf) {
        const int u = t - base;
        v[0] = s[u];
        v[1] = d1[u];
        v[2] = d2[u];
        v[3] = delta_at(d2, t, base, nf, N, denom);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(((long long)b * 4 + c) * F + f) * T + t] = from_f32<To>(v[c]);
}

template <typename To>
__global__ void __launch_bounds__(FB_THREADS)
k_fbank_norm(const float *__restrict__ q, const int *__restrict__ frame_lengths, int F, int T, long long rows, To *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (FB_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int nf = frame_lengths[r / (4LL * F)];
    const float *x = q + r * T;
    To *y = out + r * T;
    float sum = 0.f;
    for (int t = lane; t < nf; t += 64) sum += x[t];
    const float mean = wave_sum(sum) / (float)nf;
    float sq = 0.f;
    for (int t = lane; t < nf; t += 64) {
        const float d = x[t] - mean;
        sq += d * d;
    }
    const float sd = sqrtf(wave_sum(sq) / (float)nf + 1e-8f);
    for (int t = lane; t < T; t += 64) y[t] = from_f32<To>(t < nf ? (x[t] - mean) / sd : 0.f);
}

template <typename To>
int launch_delta_norm(const float *stat, const int *flen, const FbankGeom &g, int N, bool norm, void *out, float *q32, hipStream_t st)
{
    dim3 grid((unsigned)((g.T + DL_TILE - 1) / DL_TILE), (unsigned)((g.F + DL_ROWS - 1) / DL_ROWS), (unsigned)g.B);
    if (!norm) {
        hipLaunchKernelGGL(k_fbank_delta<To>, grid, dim3(FB_THREADS), 0, st, stat, flen, g.F, g.T, N, static_cast<To *>(out));
        return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(k_fbank_delta<float>, grid, dim3(FB_THREADS), 0, st, stat, flen, g.F, g.T, N, q32);
    const long long rows = 4LL * g.B * g.F;
    hipLaunchKernelGGL(k_fbank_norm<To>, dim3((unsigned)((rows + DL_ROWS - 1) / DL_ROWS)), dim3(FB_THREADS), 0, st, (const float *)q32, flen,
                       g.F, g.T, rows, static_cast<To *>(out));
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace

int fbank_tile(int L, int S) { return max(1, min(FB_TILE, (FB_SPAN_MAX - L) / S + 1)); }

size_t fbank_workspace_bytes(int B, int T, int F, bool norm)
{
    const size_t stat = ((size_t)B * F * T * 4 + 255) & ~(size_t)255;
    return stat + (norm ? (size_t)B * 4 * F * T * 4 : 0);
}

int launch_fbank(int wave_dtype, const void *wave, const int *lengths, const FbankGeom &g, int N, bool norm, int out_dtype, void *out,
                 int *frame_lengths, void *ws, hipStream_t st)
{
    if (g.nfft < 256 || g.nfft > 1024 || (g.nfft & (g.nfft - 1)) || g.L < 1 || g.L > g.nfft || g.S < 1 || g.nfilt < 1 ||
        g.nfilt > QK_FBANK_MAX_FILT || N < 1 || N > kMaxDelta)
        return QK_ERR_UNSUPPORTED;
    float *stat = static_cast<float *>(ws);
    float *q32 = reinterpret_cast<float *>(static_cast<char *>(ws) + fbank_workspace_bytes(g.B, g.T, g.F, false));
    dim3 grid((unsigned)((g.T + g.tile - 1) / g.tile), (unsigned)g.B);
    const size_t lds = fb_lds_bytes(g);
    if (wave_dtype == QK_WAVE_I16)
        hipLaunchKernelGGL(k_fbank_static<int16_t>, grid, dim3(FB_THREADS), lds, st, (const int16_t *)wave, lengths, g, stat, frame_lengths);
    else
        hipLaunchKernelGGL(k_fbank_static<float>, grid, dim3(FB_THREADS), lds, st, (const float *)wave, lengths, g, stat, frame_lengths);
    if (hipGetLastError() != hipSuccess) return QK_ERR_LAUNCH;
    switch (out_dtype) {
    case QK_F32: return launch_delta_norm<float>(stat, frame_lengths, g, N, norm, out, q32, st);
    case QK_BF16: return launch_delta_norm<bf16>(stat, frame_lengths, g, N, norm, out, q32, st);
    case QK_F16: return launch_delta_norm<f16>(stat, frame_lengths, g, N, norm, out, q32, st);
    }
    return QK_ERR_INVALID_ARG;
}

}  // namespace qk
