// Reverberation and additive noise for a batch of waveforms (batch, max_samples) -> fp32 (batch, max_samples), behind the speed
// perturbation and in front of the acoustic front end, as TWO launches (semantics: include/qk.h, "Reverberation and additive
// noise").  Every utterance draws whether it is convolved with a room impulse response of up to 8192 taps and whether a noise
// recording is added at a drawn signal-to-noise ratio; the draws are recomputed by every workgroup from workgroup-uniform values.
//
//   k_env_filter  one 256-thread workgroup per (tile of EA_TILE = 4096 outputs, utterance); the tile lies on the 16-byte grid of the
//                 output row's address.  The FIR is the hot path: Lr fused multiply-adds per output.
//     * A tile is two halves of 2048 outputs, and lane l owns outputs 8 l .. 8 l + 7 of BOTH halves.  The input window is staged
//       in LDS as float2 (x[s], x[s + 2048]), so one accumulator pair, one window pair and a splat tap make one v_pk_fma_f32:
//       the packed form is what reaches the fp32 vector peak, and pairing the halves needs no odd-aligned register pairs.
//     * Taps go through LDS in chunks of EA_JC = 512, REVERSED (tp[k] = h[j0 + 511 - k], zeros behind Lr), which turns the
//       convolution into acc[i] += tp[k] * win[p0 + i + k] with both indices ascending.  With every chunk the workgroup stages the
//       2048 + 512 window positions the chunk touches: 5120 loads for 2 M multiply-adds.  Samples outside [0, n) are staged as
//       zeros and never read; a chunk whose whole window lies outside [0, n) is skipped, and so are leading groups of 16 zero taps.
//     * A step is 8 taps: the lane holds window positions p0 + k .. p0 + k + 15 in registers (16 float2), of which the upper
//       eight are the step's four ds_read_b128 and become the next step's lower eight; the 8 taps are two wave-uniform
//       (broadcast) ds_read_b128.  64 v_pk_fma_f32 = 128 multiply-adds per 6 LDS instructions.
//     * Neighbouring lanes' windows are 64 bytes apart, a 4-way bank conflict for ds_read_b128 (16-lane groups on a 256-byte row
//       of banks).  The window is therefore stored with one 16-byte unit of padding behind every four: unit U lives at
//       U + U / 4, lane l's four units of a step at 5 (l + k / 8 + 1) + 0 .. 3, and 5 l is a bijection mod 16.
//     * Utterances that draw no reverberation, and tiles behind n, take the copy path: float(x) or +0, one element per lane and
//       pass, no LDS.
//     * The workgroup squares its valid outputs and its stretch of the wrapped noise recording in float64 and reduces both sums
//       over a fixed LDS tree into one (Es, En) partial per tile (only for utterances that draw noise).
//   k_env_mix     one workgroup per (4096 outputs, utterance that drew noise): every workgroup sums the utterance's partials in the
//                 same fixed order (lane t takes tiles t, t + 256, ..; then the tree), forms a in float64 and adds a v to r in
//                 place with one fma per sample; tile 0 writes a, Es, En into the plan row.  Not launched when no noise can fire.
//   No atomics; bit-repeatable; nothing is read on the host.
#include "qk_common.h"

namespace qk {
namespace {

constexpr int EA_THREADS = 256;
constexpr int EA_R = 8;                                         // outputs per lane and half
constexpr int EA_HALF = EA_THREADS * EA_R;
constexpr int EA_TILE = 2 * EA_HALF;                            // outputs per workgroup
constexpr int EA_JC = 512;                                      // taps per staged chunk
constexpr int EA_POS = EA_HALF + EA_JC;                         // window positions (float2) a chunk touches
constexpr int EA_UNITS = EA_POS / 2;                            // ... as 16-byte units of two positions
constexpr int EA_PAD = 1;                                       // 1: unit U at U + U / 4; 0: the unpadded layout (the A/B of DESIGN 3.16)
constexpr int EA_PUNITS = EA_UNITS + EA_PAD * (EA_UNITS / 4);
constexpr int EA_LANE = 4 + EA_PAD;                             // units from one lane's window to the next lane's
static_assert(EA_JC % 16 == 0 && EA_R == 8 && EA_UNITS % 4 == 0, "steps of 8 taps, unrolled by two; 8 positions = 4 units per lane");
static_assert(QK_REVERB_MAX_TAPS % EA_JC == 0, "whole chunks");

typedef float v2f __attribute__((ext_vector_type(2)));

struct EnvGeom {
    int B, n_max, tiles;                                        // utterances, row length, tiles per row
    qk_noise_reverb_t pol;
};

__device__ __forceinline__ unsigned fmix(unsigned h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// u(b, k) of qk.h with kb = fmix(key + b)
__device__ __forceinline__ unsigned draw(unsigned kb, unsigned k) { return fmix(kb ^ (k * 0x9E3779B1u + 0x7F4A7C15u)); }
__device__ __forceinline__ int randint(unsigned kb, unsigned k, int m) { return (int)__umulhi(draw(kb, k), (unsigned)m); }

__device__ __forceinline__ float sample_f32(float v) { return v; }
__device__ __forceinline__ float sample_f32(short v) { return (float)v; }

// the draws of utterance b and what they select (workgroup-uniform); bank lengths are clamped into the ranges qk.h asks of the caller
struct Draws {
    int n, ri, ni, o, Lr, d, Ln;
    bool do_rir, do_noise;
    float snr;
};
__device__ __forceinline__ Draws draws_of(const EnvGeom &g, int b, const int *__restrict__ lengths, const int *__restrict__ rir_len,
                                          const int *__restrict__ rir_delay, const int *__restrict__ noise_len,
                                          const unsigned *__restrict__ counter)
{
    Draws D;
    D.n = min(max(lengths[b], 0), g.n_max);
    const unsigned key = g.pol.seed + 0x9E3779B1u * (counter ? *counter : 0u);
    const unsigned kb = fmix(key + (unsigned)b);
    D.do_rir = g.pol.n_rirs > 0 && (draw(kb, 72u) >> 8) < (unsigned)g.pol.rir_prob_q24;
    D.do_noise = g.pol.n_noises > 0 && (draw(kb, 74u) >> 8) < (unsigned)g.pol.noise_prob_q24;
    D.ri = D.ni = D.o = 0;
    D.Lr = D.Ln = 1; D.d = 0;
    if (D.do_rir) {
        D.ri = randint(kb, 73u, g.pol.n_rirs);
        D.Lr = min(max(rir_len[D.ri], 1), g.pol.rir_stride);
        D.d = min(max(rir_delay[D.ri], 0), D.Lr - 1);
    }
    if (D.do_noise) {
        D.ni = randint(kb, 75u, g.pol.n_noises);
        D.Ln = min(max(noise_len[D.ni], 1), g.pol.noise_stride);
        D.o = randint(kb, 76u, D.Ln);
    }
    const float f = (float)(draw(kb, 77u) >> 8) * 0x1p-24f;
    {
#pragma clang fp contract(off)                                                   // three roundings: qk.h pins the bits of snr
        const float span = g.pol.snr_hi - g.pol.snr_lo;
        const float part = span * f;
        D.snr = g.pol.snr_lo + part;
    }
    return D;
}

// red[0 .. 255] and red[256 .. 511] each summed into their first element over a fixed tree (every thread of the workgroup calls)
__device__ __forceinline__ void reduce_pair(double *red, int tid, double a, double b)
{
    red[tid] = a; red[EA_THREADS + tid] = b;
    __syncthreads();
    for (int s = EA_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[tid] += red[tid + s];
            red[EA_THREADS + tid] += red[EA_THREADS + tid + s];
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(EA_THREADS)
k_env_filter(const T *__restrict__ wave, const int *__restrict__ lengths, const float *__restrict__ rirs, const int *__restrict__ rir_len,
             const int *__restrict__ rir_delay, const float *__restrict__ noises, const int *__restrict__ noise_len,
             const unsigned *__restrict__ counter, EnvGeom g, float *__restrict__ out, int *__restrict__ plan, double2 *__restrict__ part)
{
    __shared__ float4 xw[EA_PUNITS];
    __shared__ __attribute__((aligned(16))) float tp[EA_JC];
    __shared__ double red[2 * EA_THREADS];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.tiles), tile = (int)(blockIdx.x - (unsigned)b * g.tiles);
    const Draws D = draws_of(g, b, lengths, rir_len, rir_delay, noise_len, counter);
    const int n = D.n;
    if (tile == 0 && tid == 0 && plan) {
        int *row = plan + (long long)b * QK_NOISE_REVERB_PLAN_WORDS;
        row[0] = n; row[1] = D.do_rir ? D.ri : -1; row[2] = D.do_noise ? D.ni : -1; row[3] = D.o; row[4] = __float_as_int(D.snr);
        if (!D.do_noise) row[5] = row[6] = row[7] = 0;                        // (k_env_mix writes them otherwise)
    }

    // the tile: outputs [m_lo, m_hi) of the row, on the 16-byte grid of the row's address; [m_lo, mv) of them are valid (m < n)
    float *orow = out + (long long)b * g.n_max;
    const T *xrow = wave + (long long)b * g.n_max;
    const float *nz = noises + (long long)D.ni * g.pol.noise_stride;
    const int t0 = tile * EA_TILE - (int)((reinterpret_cast<uintptr_t>(orow) & 15) >> 2);
    const int m_lo = max(t0, 0), m_hi = min(t0 + EA_TILE, g.n_max);
    const int mv = min(m_hi, n);
    double es = 0.0, en = 0.0;

    if (D.do_rir && m_lo < mv) {
        // ---- the filter ------------------------------------------------------------------------------------------------------
        const float *h = rirs + (long long)D.ri * g.pol.rir_stride;
        const int Lr = D.Lr;
        v2f acc[EA_R];
#pragma unroll
        for (int i = 0; i < EA_R; ++i) acc[i] = v2f{0.f, 0.f};
        const float4 *xl = xw + EA_LANE * tid;
        for (int j0 = 0; j0 < Lr; j0 += EA_JC) {
            const int sbase = t0 + D.d - (j0 + EA_JC - 1);                    // the sample at window position 0, first half
            if (sbase + EA_POS + EA_HALF <= 0 || sbase >= n) continue;        // the whole window is zeros
            for (int k = tid; k < EA_JC; k += EA_THREADS) {
                const int j = j0 + EA_JC - 1 - k;
                tp[k] = j < Lr ? h[j] : 0.f;
            }
            for (int e = tid; e < EA_POS; e += EA_THREADS) {
                const int sa = sbase + e, sb = sa + EA_HALF;
                v2f w;
                w.x = (sa >= 0 && sa < n) ? sample_f32(xrow[sa]) : 0.f;
                w.y = (sb >= 0 && sb < n) ? sample_f32(xrow[sb]) : 0.f;
                const int U = e >> 1;
                reinterpret_cast<v2f *>(xw)[2 * (U + EA_PAD * (U >> 2)) + (e & 1)] = w;
            }
            __syncthreads();
            const int kstart = (EA_JC - min(EA_JC, Lr - j0)) & ~15;           // the taps in front of it are zeros
            v2f lo[8], hi[8];
            {
                const float4 *q = xl + EA_LANE * (kstart >> 3);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 v = q[c];
                    lo[2 * c] = v2f{v.x, v.y}; lo[2 * c + 1] = v2f{v.z, v.w};
                }
            }
#pragma unroll 2
            for (int k = kstart; k < EA_JC; k += 8) {
                const float4 *q = xl + EA_LANE * ((k >> 3) + 1);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 v = q[c];
                    hi[2 * c] = v2f{v.x, v.y}; hi[2 * c + 1] = v2f{v.z, v.w};
                }
                const float4 ta = *reinterpret_cast<const float4 *>(tp + k), tb = *reinterpret_cast<const float4 *>(tp + k + 4);
                const float t[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
                for (int tt = 0; tt < 8; ++tt) {
                    const v2f s = v2f{t[tt], t[tt]};
#pragma unroll
                    for (int i = 0; i < EA_R; ++i) {
                        const int idx = i + tt;
                        const v2f w = idx < 8 ? lo[idx & 7] : hi[idx & 7];
                        acc[i] = __builtin_elementwise_fma(w, s, acc[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) lo[i] = hi[i];
            }
            __syncthreads();
        }
        // ---- the lane's 2 x 8 outputs: store, and square the valid ones ----------------------------------------------------------
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int mb = t0 + half * EA_HALF + tid * EA_R;
            float v[EA_R];
#pragma unroll
            for (int i = 0; i < EA_R; ++i) {
                const float r = half ? acc[i].y : acc[i].x;
                v[i] = (mb + i >= m_lo && mb + i < mv) ? r : 0.f;
                es += (double)v[i] * (double)v[i];
            }
            if (mb >= m_lo && mb + EA_R <= m_hi) {
                *reinterpret_cast<float4 *>(orow + mb) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4 *>(orow + mb + 4) = make_float4(v[4], v[5], v[6], v[7]);
            } else {
#pragma unroll
                for (int i = 0; i < EA_R; ++i)
                    if (mb + i >= m_lo && mb + i < m_hi) orow[mb + i] = v[i];
            }
            if (D.do_noise) {
                const int ma = max(mb, m_lo), mz = min(mb + EA_R, mv);
                if (ma < mz) {
                    unsigned idx = ((unsigned)D.o + (unsigned)ma) % (unsigned)D.Ln;
                    for (int m = ma; m < mz; ++m) {
                        const float vv = nz[idx];
                        en += (double)vv * (double)vv;
                        if (++idx == (unsigned)D.Ln) idx = 0;
                    }
                }
            }
        }
    } else {
        // ---- no reverberation, or nothing valid in the tile: float(x), +0 from n on ------------------------------------------------
        for (int kk = 0; kk < EA_TILE / EA_THREADS; ++kk) {
            const int m = t0 + kk * EA_THREADS + tid;
            if (m < m_lo || m >= m_hi) continue;
            float v = 0.f;
            if (m < n) {
                v = sample_f32(xrow[m]);
                es += (double)v * (double)v;
                if (D.do_noise) {
                    const float vv = nz[((unsigned)D.o + (unsigned)m) % (unsigned)D.Ln];
                    en += (double)vv * (double)vv;
                }
            }
            orow[m] = v;
        }
    }
    if (D.do_noise) {
        reduce_pair(red, tid, es, en);
        if (tid == 0) part[(long long)b * g.tiles + tile] = make_double2(red[0], red[EA_THREADS]);
    }
}

__global__ void __launch_bounds__(EA_THREADS)
k_env_mix(const int *__restrict__ lengths, const int *__restrict__ rir_len, const int *__restrict__ rir_delay,
          const float *__restrict__ noises, const int *__restrict__ noise_len, const unsigned *__restrict__ counter, EnvGeom g,
          float *__restrict__ out, int *__restrict__ plan, const double2 *__restrict__ part)
{
    __shared__ double red[2 * EA_THREADS];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.tiles), tile = (int)(blockIdx.x - (unsigned)b * g.tiles);
    const Draws D = draws_of(g, b, lengths, rir_len, rir_delay, noise_len, counter);
    if (!D.do_noise) return;
    double es = 0.0, en = 0.0;
    for (int i = tid; i < g.tiles; i += EA_THREADS) {
        const double2 p = part[(long long)b * g.tiles + i];
        es += p.x; en += p.y;
    }
    reduce_pair(red, tid, es, en);
    const double Es = red[0], En = red[EA_THREADS];
    float a = 0.f;
    if (Es > 0.0 && En > 0.0) a = (float)(sqrt(Es / En) * pow(10.0, -(double)D.snr / 20.0));
    if (tile == 0 && tid == 0 && plan) {
        int *row = plan + (long long)b * QK_NOISE_REVERB_PLAN_WORDS;
        row[5] = __float_as_int(a); row[6] = __float_as_int((float)Es); row[7] = __float_as_int((float)En);
    }
    if (a == 0.f) return;
    float *orow = out + (long long)b * g.n_max;
    const float *nz = noises + (long long)D.ni * g.pol.noise_stride;
    const int m_end = min(tile * EA_TILE + EA_TILE, D.n);
    for (int m = tile * EA_TILE + tid; m < m_end; m += EA_THREADS)
        orow[m] = fmaf(a, nz[((unsigned)D.o + (unsigned)m) % (unsigned)D.Ln], orow[m]);
}

int env_tiles(int n_max) { return (n_max + 3 + EA_TILE - 1) / EA_TILE; }         // a row's first tile may start up to 3 floats early

}  // namespace

size_t noise_reverb_workspace_bytes(int B, int n_max) { return (size_t)B * (size_t)env_tiles(n_max) * sizeof(double2); }

int launch_noise_reverb(int wave_dtype, int B, int n_max, const void *wave, const int *lengths, const qk_noise_reverb_t &pol,
                        const float *rirs, const int *rir_len, const int *rir_delay, const float *noises, const int *noise_len,
                        const unsigned *counter, float *out, int *plan, void *ws, hipStream_t st)
{
    EnvGeom g;
    g.B = B; g.n_max = n_max; g.tiles = env_tiles(n_max);
    if ((long long)g.tiles * B > INT_MAX) return QK_ERR_UNSUPPORTED;
    g.pol = pol;
    const dim3 grid((unsigned)(g.tiles * B)), block(EA_THREADS);
    double2 *part = static_cast<double2 *>(ws);
    if (wave_dtype == QK_WAVE_I16)
        hipLaunchKernelGGL((k_env_filter<short>), grid, block, 0, st, static_cast<const short *>(wave), lengths, rirs, rir_len, rir_delay,
                           noises, noise_len, counter, g, out, plan, part);
    else
        hipLaunchKernelGGL((k_env_filter<float>), grid, block, 0, st, static_cast<const float *>(wave), lengths, rirs, rir_len, rir_delay,
                           noises, noise_len, counter, g, out, plan, part);
    if (hipGetLastError() != hipSuccess) return QK_ERR_LAUNCH;
    if (pol.n_noises > 0 && pol.noise_prob_q24 > 0) {
        hipLaunchKernelGGL(k_env_mix, grid, block, 0, st, lengths, rir_len, rir_delay, noises, noise_len, counter, g, out, plan,
                           static_cast<const double2 *>(part));
        if (hipGetLastError() != hipSuccess) return QK_ERR_LAUNCH;
    }
    return 0;
}

}  // namespace qk
