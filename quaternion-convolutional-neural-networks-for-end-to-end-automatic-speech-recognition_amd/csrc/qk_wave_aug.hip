// Speed and volume perturbation of a batch of waveforms (batch, max_samples) -> fp32 (batch, out_samples), in front of the acoustic
// front end, as ONE launch (semantics: include/qk.h, "Speed and volume perturbation").  Every utterance is resampled by one of the
// policy's speeds p/q with a host-built polyphase windowed-sinc table (q phases of 2 Kw + 2 taps) and multiplied by a drawn gain.
//
//   k_speed_perturb  one 256-thread workgroup per (tile of SP_TILE output samples, utterance).  The tile lies on the 16-byte grid of
//                    the output row's address, so its chunks of four outputs are whole 16-byte stores; the chunk that the row's
//                    start or end clips is stored element by element.
//     1. every thread derives the utterance's two draws (speed index, gain) and n' -- a handful of integer operations on
//        workgroup-uniform values; thread 0 of tile 0 stores out_lengths and the plan row.
//     2. a tile that holds valid outputs (m < n') stages its input window as fp32 in LDS: input samples i0(first) - Kw ..
//        i0(last) + Kw + 1, fetched as 16-byte chunks on the grid of the input row's address and stored as 16-byte LDS writes; a
//        chunk that crosses sample 0 or sample n is assembled element by element, zero outside [0, n) -- samples >= n are never
//        read.  The tile's windows overlap their neighbours' by 2 Kw + 2 samples and the chunk slack, about 1 % of a tile.  The
//        utterance's q x taps table goes to LDS with a phase stride of taps + 1 floats: taps is even, the stride odd, so the
//        q <= 32 phases start on different banks.
//     3. four outputs per lane and pass.  While it COMPUTES, lane l of a wave takes outputs 64 k + l (k = 0 .. 3) of the wave's 256:
//        neighbouring lanes then read neighbouring window samples (lane stride p/q floats), where four CONSECUTIVE outputs per
//        lane would put the lanes 4 p/q floats apart, a 3- to 4-way bank conflict on every tap.  The 256 results are transposed
//        through LDS (four 4-byte writes, one 16-byte read), so that every lane STORES four consecutive outputs as 16 bytes.
//        Outputs m >= n' are zeros; a tile past n' reads no input at all.
//   No atomics, no workspace, no synchronisation; the taps of one output are summed in ascending j with fused multiply-adds.
#include "qk_common.h"

namespace qk {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_TILE = 2048;                                   // outputs per workgroup: two passes of four per lane
constexpr int SP_PASS = SP_THREADS * 4;
// floats of the staged window: i0 moves by at most 2 (SP_TILE - 1) + 1 over a tile (p/q <= 2), plus the taps, plus up to 7
// samples of chunk slack at either end
constexpr int SP_WIN = 2 * SP_TILE + QK_SPEED_MAX_TAPS + 16;
constexpr int SP_TAB = QK_SPEED_MAX_DEN * (QK_SPEED_MAX_TAPS + 1);
static_assert(SP_TILE % SP_PASS == 0, "a tile is a whole number of passes");

struct SpeedGeom {
    int B, n_max, n_out, tiles;                                 // utterances, input and output row length, tiles per row
    unsigned q_mul[QK_SPEED_MAX_SPEEDS], q_shr[QK_SPEED_MAX_SPEEDS];          // fastdiv by den[i]
    qk_speed_perturb_t pol;
};

__device__ __forceinline__ unsigned fmix(unsigned h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// u(b, k) of qk.h with kb = fmix(key + b)
__device__ __forceinline__ unsigned draw(unsigned kb, unsigned k) { return fmix(kb ^ (k * 0x9E3779B1u + 0x7F4A7C15u)); }

__device__ __forceinline__ float sample_f32(float v) { return v; }
__device__ __forceinline__ float sample_f32(short v) { return (float)v; }

// the 16 bytes at p (16-byte aligned) as 16 / sizeof(T) floats
__device__ __forceinline__ void load_chunk(const float *p, float (&v)[4])
{
    const float4 c = *reinterpret_cast<const float4 *>(p);
    v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
}
__device__ __forceinline__ void load_chunk(const short *p, float (&v)[8])
{
    const uint4 c = *reinterpret_cast<const uint4 *>(p);
    const unsigned w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = (float)(short)(w[j] & 0xffffu);
        v[2 * j + 1] = (float)(short)(w[j] >> 16);
    }
}

template <typename T>
__global__ void __launch_bounds__(SP_THREADS)
k_speed_perturb(const T *__restrict__ wave, const int *__restrict__ lengths, const float *__restrict__ tables,
                const unsigned *__restrict__ counter, SpeedGeom g, float *__restrict__ out, int *__restrict__ out_lengths,
                int *__restrict__ plan)
{
    constexpr int VI = 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) float win[SP_WIN];
    __shared__ __attribute__((aligned(16))) float turn[SP_PASS];
    __shared__ float tab[SP_TAB];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.tiles), tile = (int)(blockIdx.x - (unsigned)b * g.tiles);

    // ---- 1. the utterance's draws and lengths (workgroup-uniform) -------------------------------------------------------------
    const int n = min(max(lengths[b], 0), g.n_max);
    const unsigned key = g.pol.seed + 0x9E3779B1u * (counter ? *counter : 0u);
    const unsigned kb = fmix(key + (unsigned)b);
    const int i = (int)__umulhi(draw(kb, 64u), (unsigned)g.pol.n_speeds);
    const float f = (float)(draw(kb, 65u) >> 8) * 0x1p-24f;
    const float gain = __fadd_rn(g.pol.gain_lo, __fmul_rn(__fsub_rn(g.pol.gain_hi, g.pol.gain_lo), f));
    const int p = g.pol.num[i], q = g.pol.den[i], Kw = g.pol.half_width[i];
    const unsigned q_mul = g.q_mul[i], q_shr = g.q_shr[i];
    const int np = (int)(((unsigned)n * (unsigned)q + (unsigned)p - 1u) / (unsigned)p);          // n q < 2^31
    if (tile == 0 && tid == 0) {
        out_lengths[b] = np;
        if (plan) {
            int *row = plan + (long long)b * QK_SPEED_PLAN_WORDS;
            row[0] = n; row[1] = i; row[2] = np; row[3] = __float_as_int(gain);
        }
    }

    // the tile: outputs [m_lo, m_hi) of the row, on the 16-byte grid of the row's address; [m_lo, mv) of them are valid (m < n')
    float *orow = out + (long long)b * g.n_out;
    const int t0 = tile * SP_TILE - (int)((reinterpret_cast<uintptr_t>(orow) & 15) >> 2);
    const int m_lo = max(t0, 0), m_hi = min(t0 + SP_TILE, g.n_out);
    if (m_lo >= m_hi) return;
    const int mv = min(m_hi, np);
    const bool filt = p != q;
    const int taps = 2 * Kw + 2, ts = taps + 1;
    int wbase = 0;

    // ---- 2. stage the input window and the table ------------------------------------------------------------------------------
    if (m_lo < mv) {
        const int w0 = fastdiv(m_lo * p, q_mul, q_shr) - Kw, w1 = fastdiv((mv - 1) * p, q_mul, q_shr) + Kw + 2;     // samples [w0, w1)
        const T *xrow = wave + (long long)b * g.n_max;
        const int ishift = (int)((reinterpret_cast<uintptr_t>(xrow) & 15) / sizeof(T));
        wbase = ((w0 + ishift + 64) & ~(VI - 1)) - 64 - ishift;              // <= w0, a chunk start (w0 >= -Kw > -64)
        const int nchunk = (w1 - wbase + VI - 1) / VI;                       // nchunk VI <= SP_WIN
        for (int c = tid; c < nchunk; c += SP_THREADS) {
            const int e0 = wbase + c * VI;
            float v[VI];
            if (e0 >= 0 && e0 + VI <= n) {
                load_chunk(xrow + e0, v);
            } else {
#pragma unroll
                for (int j = 0; j < VI; ++j) {
                    const int e = e0 + j;
                    v[j] = (e >= 0 && e < n) ? sample_f32(xrow[e]) : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < VI; j += 4) *reinterpret_cast<float4 *>(&win[c * VI + j]) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
        }
        if (filt) {
            const float *src = tables + g.pol.table_offset[i];
            for (int k = tid; k < q * taps; k += SP_THREADS) {
                const int r = k / taps;
                tab[r * ts + (k - r * taps)] = src[k];
            }
        }
    }
    __syncthreads();

    // ---- 3. the outputs -------------------------------------------------------------------------------------------------------
    const int wv = tid & ~63, lane = tid & 63;
    for (int pass = 0; pass < SP_TILE / SP_PASS; ++pass) {
        const int pb = t0 + pass * SP_PASS;                                   // the pass's first output
        if (pb >= m_hi) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int m = pb + wv * 4 + 64 * k + lane;
            float y = 0.f;
            if (m >= m_lo && m < mv) {
                float acc;
                if (filt) {
                    const int num = m * p;                                    // < 2^31
                    const int i0 = fastdiv(num, q_mul, q_shr), r = num - i0 * q;
                    const float *xs = win + (i0 - Kw - wbase), *h = tab + r * ts;
                    acc = 0.f;
                    for (int j = 0; j < taps; j += 2) {
                        acc = fmaf(h[j], xs[j], acc);
                        acc = fmaf(h[j + 1], xs[j + 1], acc);
                    }
                } else {
                    acc = win[m - wbase];
                }
                y = gain * acc;
            }
            turn[wv * 4 + 64 * k + lane] = y;
        }
        __syncthreads();
        const float4 o = *reinterpret_cast<const float4 *>(&turn[tid * 4]);
        const int m0 = pb + tid * 4;
        if (m0 >= m_lo && m0 + 4 <= m_hi) {
            *reinterpret_cast<float4 *>(orow + m0) = o;
        } else {
            const float e[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (m0 + c >= m_lo && m0 + c < m_hi) orow[m0 + c] = e[c];
        }
    }
}

template <typename T>
int launch_t(const void *wave, const int *lengths, const float *tables, const unsigned *counter, const SpeedGeom &g, float *out,
             int *out_lengths, int *plan, hipStream_t st)
{
    hipLaunchKernelGGL((k_speed_perturb<T>), dim3((unsigned)(g.tiles * g.B)), dim3(SP_THREADS), 0, st, static_cast<const T *>(wave), lengths,
                       tables, counter, g, out, out_lengths, plan);
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace

int launch_speed_perturb(int wave_dtype, int B, int n_max, const void *wave, const int *lengths, const qk_speed_perturb_t &pol,
                         const float *tables, const unsigned *counter, int n_out, float *out, int *out_lengths, int *plan,
                         hipStream_t st)
{
    SpeedGeom g;
    g.B = B; g.n_max = n_max; g.n_out = n_out;
    g.tiles = (n_out + 3 + SP_TILE - 1) / SP_TILE;                            // a row's first chunk may start up to 3 floats early
    if ((long long)g.tiles * B > INT_MAX) return QK_ERR_UNSUPPORTED;
    g.pol = pol;
    for (int i = 0; i < QK_SPEED_MAX_SPEEDS; ++i) {
        g.q_mul[i] = g.q_shr[i] = 0;
        if (i < pol.n_speeds) fastdiv_of((unsigned)pol.den[i], &g.q_mul[i], &g.q_shr[i]);
    }
    if (wave_dtype == QK_WAVE_I16) return launch_t<short>(wave, lengths, tables, counter, g, out, out_lengths, plan, st);
    return launch_t<float>(wave, lengths, tables, counter, g, out, out_lengths, plan, st);
}

}  // namespace qk
