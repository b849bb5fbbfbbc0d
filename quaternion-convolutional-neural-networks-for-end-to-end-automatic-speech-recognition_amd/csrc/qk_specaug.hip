// SpecAugment on the model's channels_first quaternion input (batch, planes, rows, frames): time warp, frequency masks and time
// masks as ONE launch (semantics: include/qk.h, "SpecAugment").  The four planes of a time-frequency cell are one quaternion, so
// every plane of an utterance gets the same warp and the same masks.
//
//   k_spec_augment  one 256-thread workgroup per (group of G consecutive rows of the (planes x rows) rows, utterance).  Consecutive
//                   rows are contiguous, so the group is ONE span of G x frames elements.
//     1. 17 threads derive the utterance's draws (one per mask, one for the warp) into a 36-word plan in LDS; the workgroup of
//        group 0 also stores the plan row.
//     2. STAGED (the policy warps and a row fits the LDS budget): the span's input is copied to LDS as raw 16-byte chunks (aligned
//        chunks with 16-byte loads, the clipped chunk at either end element by element); chunks that lie in the valid frames of a
//        frequency-masked row are not loaded.  Every input element is read from memory once.
//     3. Output: each lane owns the 16-byte-aligned chunks of `out` that meet the span -- V = 16 / sizeof(out element) frames, decoded
//        to (row, t) with one division per chunk -- forms fill / warped value / copy per frame in fp32 and stores the chunk with one
//        16-byte store (a chunk clipped by the span's end is stored element by element; the neighbouring workgroup writes the rest).
//        The warp's two taps come from LDS (STAGED), else from memory: an unwarped utterance then reads its chunk with 16-byte
//        loads where the input's alignment allows, and skips the load of a chunk that is masked as a whole.
//   No atomics, no workspace; a row of any length is served (rows beyond the LDS budget gather their taps from memory).
#include "qk_common.h"

namespace qk {
namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_LDS_BUDGET = 48 * 1024;      // staged span, bytes
constexpr int SA_M = QK_SPECAUG_MAX_MASKS;

struct SpecAugGeom {
    int B, PR, R, T;                // utterances, planes x rows, rows, frames
    int G, groups;                  // rows per workgroup, workgroups per utterance
    unsigned t_mul, t_shr, r_mul, r_shr;      // fastdiv by T and by R
    qk_specaug_t pol;
};

__device__ __forceinline__ unsigned fmix(unsigned h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// randint(b, k, m) of qk.h with kb = fmix(key + b)
__device__ __forceinline__ int randint(unsigned kb, unsigned k, int m) { return (int)__umulhi(fmix(kb ^ (k * 0x9E3779B1u + 0x7F4A7C15u)), (unsigned)m); }

template <typename T> __device__ __forceinline__ float bits_to_f32(unsigned v);
template <> __device__ __forceinline__ float bits_to_f32<float>(unsigned v) { return __uint_as_float(v); }
template <> __device__ __forceinline__ float bits_to_f32<bf16>(unsigned v) { return __uint_as_float(v << 16); }
template <> __device__ __forceinline__ float bits_to_f32<f16>(unsigned v)
{
    union { unsigned short u; f16 h; } c;
    c.u = (unsigned short)v;
    return (float)c.h;
}
template <typename T> __device__ __forceinline__ unsigned f32_to_bits(float v);
template <> __device__ __forceinline__ unsigned f32_to_bits<float>(float v) { return __float_as_uint(v); }
template <> __device__ __forceinline__ unsigned f32_to_bits<bf16>(float v) { return from_f32<bf16>(v).x; }
template <> __device__ __forceinline__ unsigned f32_to_bits<f16>(float v)
{
    union { unsigned short u; f16 h; } c;
    c.h = (f16)v;
    return c.u;
}

// V consecutive elements at p as floats: vector loads of min(16, V sizeof(T)) bytes when p is aligned to that, else element loads
template <typename T, int V>
__device__ __forceinline__ void load_vec(const T *p, float (&o)[V])
{
    constexpr int BYTES = V * (int)sizeof(T), W = BYTES < 16 ? BYTES : 16;
    if ((reinterpret_cast<uintptr_t>(p) & (W - 1)) == 0) {
        unsigned w[BYTES / 4];
        if constexpr (W == 8) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            w[0] = v.x; w[1] = v.y;
        } else {
#pragma unroll
            for (int q = 0; q < BYTES / 16; ++q) {
                const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if constexpr (sizeof(T) == 4) o[j] = bits_to_f32<T>(w[j]);
            else o[j] = bits_to_f32<T>((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = to_f32(p[j]);
    }
}

template <typename Tin, typename To, bool STAGED>
__global__ void __launch_bounds__(SA_THREADS)
k_spec_augment(const Tin *__restrict__ x, const int *__restrict__ lengths, const unsigned *__restrict__ counter, SpecAugGeom g,
               To *__restrict__ out, int *__restrict__ plan)
{
    constexpr int V = 16 / (int)sizeof(To), VI = 16 / (int)sizeof(Tin);
    extern __shared__ uint4 sa_smem[];
    __shared__ int pl[QK_SPECAUG_PLAN_WORDS];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.groups), grp = (int)(blockIdx.x - (unsigned)b * g.groups);
    const int T = g.T, R = g.R;
    const int n = min(max(lengths[b], 0), T);

    // ---- 1. the utterance's draws ------------------------------------------------------------------------------------------
    if (tid < 2 * SA_M + 1) {
        const unsigned key = g.pol.seed + 0x9E3779B1u * (counter ? *counter : 0u);
        const unsigned kb = fmix(key + (unsigned)b);
        if (tid < SA_M) {                                     // frequency mask tid
            int f0 = 0, fw = 0;
            if (tid < g.pol.freq_masks) {
                fw = randint(kb, 2 + 2 * tid, min(g.pol.freq_width, R) + 1);
                f0 = randint(kb, 3 + 2 * tid, R - fw + 1);
            }
            pl[4 + 2 * tid] = f0; pl[5 + 2 * tid] = fw;
        } else if (tid < 2 * SA_M) {                          // time mask i
            const int i = tid - SA_M;
            int t0 = 0, tw = 0;
            if (i < g.pol.time_masks) {
                const int cap = min(g.pol.time_width, (int)floorf((float)n * g.pol.time_ratio));
                tw = randint(kb, 18 + 2 * i, cap + 1);
                t0 = randint(kb, 19 + 2 * i, n - tw + 1);
            }
            pl[4 + 2 * SA_M + 2 * i] = t0; pl[5 + 2 * SA_M + 2 * i] = tw;
        } else {                                              // the warp
            const int W = g.pol.time_warp;
            int c = 0, w = 0;
            if (W >= 1 && n >= 3 && W <= (n - 3) / 2) {       // n >= 2 W + 3
                c = W + 1 + randint(kb, 0, n - 2 * W - 2);
                w = randint(kb, 1, 2 * W + 1) - W;
            }
            pl[0] = n; pl[1] = c; pl[2] = w; pl[3] = 0;
        }
    }
    __syncthreads();
    if (grp == 0 && plan && tid < QK_SPECAUG_PLAN_WORDS) plan[(long long)b * QK_SPECAUG_PLAN_WORDS + tid] = pl[tid];

    const int c = pl[1], cp = c + pl[2];
    const bool active = c > 0;
    const int nfm = g.pol.freq_masks, ntm = g.pol.time_masks;
    const float fill = g.pol.fill;
    auto row_masked = [&](int row) {                         // row in [0, PR)
        const int r = row - fastdiv(row, g.r_mul, g.r_shr) * R;
        bool m = false;
        for (int i = 0; i < nfm; ++i) m |= (unsigned)(r - pl[4 + 2 * i]) < (unsigned)pl[5 + 2 * i];
        return m;
    };
    auto frame_masked = [&](int t) {
        bool m = false;
        for (int i = 0; i < ntm; ++i) m |= (unsigned)(t - pl[4 + 2 * SA_M + 2 * i]) < (unsigned)pl[5 + 2 * SA_M + 2 * i];
        return m;
    };

    // the span: elements [s0, s1) of the utterance's PR x T block
    const int row0 = grp * g.G, row1 = min(row0 + g.G, g.PR);
    const int s0 = row0 * T, s1 = row1 * T;
    const long long u0 = (long long)b * g.PR * T;
    const Tin *xu = x + u0;
    To *ou = out + u0;

    // ---- 2. stage the span's input in LDS, raw, on the 16-byte grid of its address --------------------------------------------
    const int in_shift = (int)((reinterpret_cast<uintptr_t>(xu + s0) & 15) / sizeof(Tin));      // the span's first element in its chunk
    const Tin *lds = reinterpret_cast<const Tin *>(sa_smem) + in_shift - s0;                   // lds[e] = element e of the utterance
    if constexpr (STAGED) {
        Tin *ldw = reinterpret_cast<Tin *>(sa_smem) + in_shift - s0;
        const int nchunk = (in_shift + (s1 - s0) + VI - 1) / VI;
        for (int k = tid; k < nchunk; k += SA_THREADS) {
            const int e0 = s0 - in_shift + k * VI;            // first element of the chunk (may lie before s0)
            const int lo = max(e0, s0), hi = min(e0 + VI, s1) - 1;
            const int rlo = fastdiv(lo, g.t_mul, g.t_shr), rhi = fastdiv(hi, g.t_mul, g.t_shr);
            if (rlo == rhi && hi - rhi * T < n && row_masked(rlo)) continue;        // valid frames of a masked row: never read
            if (lo == e0 && hi == e0 + VI - 1) {
                sa_smem[k] = *reinterpret_cast<const uint4 *>(xu + e0);
            } else {
                for (int e = lo; e <= hi; ++e) ldw[e] = xu[e];
            }
        }
        __syncthreads();
    }

    // ---- 3. the output chunks that meet the span --------------------------------------------------------------------------------
    const int out_shift = (int)((reinterpret_cast<uintptr_t>(ou + s0) & 15) / sizeof(To));
    const int nchunk = (out_shift + (s1 - s0) + V - 1) / V;
    const bool wide = n > 32767;                              // 2 n^2 no longer fits 32 bits
    for (int k = tid; k < nchunk; k += SA_THREADS) {
        const int e0 = s0 - out_shift + k * V;
        const int lo = max(e0, s0), hi = min(e0 + V, s1) - 1;
        const bool full = lo == e0 && hi == e0 + V - 1;
        int row = fastdiv(lo, g.t_mul, g.t_shr), t = lo - row * T;
        bool rm = row_masked(row);
        float v[V];
        bool direct = false;                                  // v already holds the chunk's input
        if (!STAGED && full && !active) {
            // unwarped, from memory: one vector load, unless every frame of the chunk is masked
            const int rhi = fastdiv(hi, g.t_mul, g.t_shr);
            bool need = rhi != row || hi - rhi * T >= n || !rm;
            if (need && rm == false && rhi == row && ntm) {
                need = false;
                for (int j = 0; j < V; ++j) need |= !frame_masked(t + j);
            }
            if (need) load_vec<Tin, V>(xu + e0, v);
            direct = true;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int e = e0 + j;
            if (e >= lo && e <= hi) {
                float y;
                if (t >= n) {
                    y = direct ? v[j] : (STAGED ? to_f32(lds[e]) : to_f32(xu[e]));
                } else if (rm || frame_masked(t)) {
                    y = fill;
                } else if (!active) {
                    y = direct ? v[j] : (STAGED ? to_f32(lds[e]) : to_f32(xu[e]));
                } else {
                    int i0, r, den;
                    if (!wide) {
                        unsigned num;
                        if (t <= cp) { num = (unsigned)t * (unsigned)c; den = cp; }
                        else { num = (unsigned)c * (unsigned)(n - 1 - cp) + (unsigned)(t - cp) * (unsigned)(n - 1 - c); den = n - 1 - cp; }
                        i0 = (int)(num / (unsigned)den);
                        r = (int)(num - (unsigned)i0 * (unsigned)den);
                    } else {
                        unsigned long long num;
                        if (t <= cp) { num = (unsigned long long)t * c; den = cp; }
                        else { num = (unsigned long long)c * (n - 1 - cp) + (unsigned long long)(t - cp) * (n - 1 - c); den = n - 1 - cp; }
                        i0 = (int)(num / (unsigned long long)den);
                        r = (int)(num - (unsigned long long)i0 * den);
                    }
                    const int base = e - t;                   // the row's frame 0
                    const float x0 = STAGED ? to_f32(lds[base + i0]) : to_f32(xu[base + i0]);
                    y = x0;
                    if (r) {                                  // (r == 0: the input itself, bit for bit)
                        const int i1 = min(i0 + 1, n - 1);
                        const float x1 = STAGED ? to_f32(lds[base + i1]) : to_f32(xu[base + i1]);
                        y = x0 + ((float)r / (float)den) * (x1 - x0);
                    }
                }
                v[j] = y;
                if (++t == T) { t = 0; ++row; rm = row < row1 ? row_masked(row) : false; }
            }
        }
        if (full) {
            unsigned w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (sizeof(To) == 4) w[q] = f32_to_bits<To>(v[q]);
                else w[q] = f32_to_bits<To>(v[2 * q]) | (f32_to_bits<To>(v[2 * q + 1]) << 16);
            }
            *reinterpret_cast<uint4 *>(ou + e0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (e0 + j >= lo && e0 + j <= hi) ou[e0 + j] = from_f32<To>(v[j]);
        }
    }
}

template <typename Tin, typename To>
int launch_t(const void *x, const int *lengths, const unsigned *counter, SpecAugGeom g, void *out, int *plan, hipStream_t st)
{
    constexpr int V = 16 / (int)sizeof(To);
    const int T = g.T;
    // rows per workgroup: about two output chunks per lane, within the LDS budget when staged
    long long G = ((long long)SA_THREADS * V * 2 + T - 1) / T;
    G = max(1LL, min(G, (long long)g.PR));
    const long long row_bytes = (long long)T * (long long)sizeof(Tin);
    const bool staged = g.pol.time_warp >= 1 && row_bytes + 32 <= SA_LDS_BUDGET;
    if (staged) G = min(G, (SA_LDS_BUDGET - 32) / row_bytes);
    g.G = (int)G;
    g.groups = (g.PR + g.G - 1) / g.G;
    if ((long long)g.groups * g.B > INT_MAX) return QK_ERR_UNSUPPORTED;
    fastdiv_of((unsigned)T, &g.t_mul, &g.t_shr);
    fastdiv_of((unsigned)g.R, &g.r_mul, &g.r_shr);
    const dim3 grid((unsigned)(g.groups * g.B));
    if (staged) {
        const size_t lds = ((size_t)g.G * row_bytes + 32 + 15) & ~(size_t)15;
        hipLaunchKernelGGL((k_spec_augment<Tin, To, true>), grid, dim3(SA_THREADS), lds, st, static_cast<const Tin *>(x), lengths, counter, g,
                           static_cast<To *>(out), plan);
    } else {
        hipLaunchKernelGGL((k_spec_augment<Tin, To, false>), grid, dim3(SA_THREADS), 0, st, static_cast<const Tin *>(x), lengths, counter, g,
                           static_cast<To *>(out), plan);
    }
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

template <typename Tin>
int launch_in(int out_dtype, const void *x, const int *lengths, const unsigned *counter, const SpecAugGeom &g, void *out, int *plan,
              hipStream_t st)
{
    switch (out_dtype) {
    case QK_F32: return launch_t<Tin, float>(x, lengths, counter, g, out, plan, st);
    case QK_BF16: return launch_t<Tin, bf16>(x, lengths, counter, g, out, plan, st);
    case QK_F16: return launch_t<Tin, f16>(x, lengths, counter, g, out, plan, st);
    }
    return QK_ERR_INVALID_ARG;
}

}  // namespace

int launch_spec_augment(int in_dtype, int out_dtype, int B, int P, int R, int T, const void *x, const int *lengths,
                        const qk_specaug_t &pol, const unsigned *counter, void *out, int *plan, hipStream_t st)
{
    SpecAugGeom g;
    g.B = B; g.PR = P * R; g.R = R; g.T = T;
    g.G = 1; g.groups = g.PR;
    g.t_mul = g.t_shr = g.r_mul = g.r_shr = 0;
    g.pol = pol;
    switch (in_dtype) {
    case QK_F32: return launch_in<float>(out_dtype, x, lengths, counter, g, out, plan, st);
    case QK_BF16: return launch_in<bf16>(out_dtype, x, lengths, counter, g, out, plan, st);
    case QK_F16: return launch_in<f16>(out_dtype, x, lengths, counter, g, out, plan, st);
    }
    return QK_ERR_INVALID_ARG;
}

}  // namespace qk
