// K.ctc_decode (greedy and beam search) and tf.edit_distance on the model's posteriors -- what turns the validation function of the
// reference (models/interspeech_model.py:182-185: val_function = K.function([I], [pred])) into a phone error rate.
//
// Inputs are the softmax outputs y_pred (B, T, C), blank = C - 1; u[t][c] = log(y_pred[t][c] + 1e-7) (Keras' epsilon()); only the
// first Tn = min(max(input_length[b], 0), T) frames count (the clamp of qk_ctc.hip).  Semantics in full: include/qk.h, "CTC decoding".
//
//   k_ctc_greedy     one wave per sample: per frame a wave argmax (lowest index on ties), the emitted labels (a change of symbol that
//                    is not the blank) compacted by ballot + prefix count; log_prob = -sum_t max_c u[t][c] (TensorFlow's sign).
//   k_ctc_beam       one 256-thread workgroup per sample: CTC prefix beam search without a language model, beam state in LDS, the
//                    top beam_width of the stay / extension candidates chosen by a radix select over order-preserving 48-bit keys
//                    (32-bit score, 16-bit tie rank) -- the candidates are recomputed on every pass instead of being stored, so the
//                    LDS footprint does not grow with the class count.  Every kept beam writes one history word per frame (source slot,
//                    appended label) to the workspace; the paths are read back from it after the last frame.
//                    LM = true fuses a phone n-gram LM (orders 1-3, dense natural-log table (C^(order-1), C)): candidates are ranked by
//                    S = tot + F, F = alpha log P_LM(prefix) + beta |prefix| carried per beam in dynamic LDS with the label before
//                    `last`.  The LM value of an extension (beam k, class c) comes from LDS on every select pass: the whole table when it
//                    fits in 64 KB, otherwise the row of each live beam's context, staged once per frame.  With eos the final beams are
//                    re-ranked by S + alpha log P(</s> | prefix) by a counting rank before the backtrack.
//   k_edit_distance  one wave per pair: Levenshtein distance row by row over the hypothesis, vectorised over the reference, the
//                    insertion chain along a row as a wave prefix-min: D[j] = j + min_{k <= j} (tmp[k] - k).
#include "qk_seq.h"
#include <climits>

namespace qk {
namespace {

constexpr float kEps = 1e-7f;          // keras.backend.epsilon()
constexpr int BEAM_THREADS = 256;
constexpr int kMaxBeam = 128;
constexpr int kMaxClasses = 256;
constexpr int kMaxEditRef = 1024;
constexpr int kMaxLmOrder = 3;
constexpr int kMaxLmTrigramClasses = 64;
constexpr size_t kLmWholeTableBytes = 64 * 1024;      // the whole LM table goes to LDS up to this size, else per-beam context rows
constexpr size_t kLmMaxDynLds = 128 * 1024 + 3 * 1024;  // dynamic LDS of the LM variant (the static part is ~20 KB of the 160 KB)

__device__ __forceinline__ float lse2f(float a, float b)
{
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(fminf(a, b) - m));
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane)
{
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// ---- greedy ---------------------------------------------------------------------------------------------------------------------
// One wave (= one workgroup) per sample.  Frames are taken 64 at a time: lane j ends up holding the argmax of frame t0 + j, so the
// emission test (symbol changed, not blank) and the compaction are one shuffle and one ballot per 64 frames.  The row loads of 8 frames
// are issued before their reductions.
template <typename T>
__global__ void __launch_bounds__(64)
k_ctc_greedy(const T *__restrict__ pred, const int *__restrict__ in_len, int B, int T_, int C, int *__restrict__ decoded,
             int *__restrict__ dlen, float *__restrict__ logp)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tn = min(max(in_len[b], 0), T_);
    const int blank = C - 1;
    const T *p = pred + (long long)b * T_ * C;
    int *row = decoded + (long long)b * T_;
    int count = 0, prevk = -1;
    float lsum = 0.f;
    for (int t0 = 0; t0 < Tn; t0 += 64) {
        const int nf = min(64, Tn - t0);
        int myk = -1;
        float myv = 0.f;
        for (int j0 = 0; j0 < nf; j0 += 8) {
            float v[8][4];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = lane + 64 * q;
                    v[jj][q] = (j0 + jj < nf && c < C) ? to_f32(p[(long long)(t0 + j0 + jj) * C + c]) : -INFINITY;
                }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                float best = -INFINITY;
                int bi = INT_MAX;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (v[jj][q] > best || (bi == INT_MAX && lane + 64 * q < C)) { best = v[jj][q]; bi = lane + 64 * q; }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const float ov = __shfl_xor(best, d, 64);
                    const int oi = __shfl_xor(bi, d, 64);
                    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
                }
                if (lane == j0 + jj) { myk = bi; myv = best; }
            }
        }
        const bool valid = lane < nf;
        int prevlane = __shfl_up(myk, 1, 64);
        if (lane == 0) prevlane = prevk;
        const bool emit = valid && myk != blank && myk != prevlane;
        const unsigned long long mask = __ballot(emit);
        if (emit) row[count + lanes_below(mask, lane)] = myk;
        count += __popcll(mask);
        prevk = __shfl(myk, nf - 1, 64);
        if (valid) lsum += logf(myv + kEps);
    }
    lsum = wave_sum(lsum);
    for (int i = count + lane; i < T_; i += 64) row[i] = -1;
    if (lane == 0) { dlen[b] = count; logp[b] = -lsum; }
}

// ---- beam search ------------------------------------------------------------------------------------------------------------------
// Prefix identity: a 64-bit hash of the label sequence, h(l + c) = mix(h(l), c), h(empty) = 0, with a splitmix64 finaliser; a beam
// also keeps its parent's hash.  The merge test "extension l + c is beam m" is h(l) == parent hash of m and c == last(m): two distinct
// prefixes pass it only by a 64-bit collision, ~2^-64 per comparison; a decode makes at most Tn x beam_width^2 of them (2e6 at
// T = 200, W = 100: < 1e-13 per sample).
__device__ __forceinline__ unsigned long long hmix(unsigned long long h, int c)
{
    unsigned long long z = h + 0x9E3779B97F4A7C15ull * (unsigned long long)(c + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Candidate order: higher total first; on equal totals stay before extension, then lower source slot, then lower class.  As one
// unsigned 48-bit key, larger = better: the score's order-preserving bits above 0xFFFF - (ext << 15 | slot << 8 | class).
__device__ __forceinline__ unsigned long long cand_key(float s, unsigned sec)
{
    s += 0.0f;                                         // -0 -> +0
    unsigned u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 16) | (0xFFFFu - sec);
}

struct BeamSet {
    float pb[kMaxBeam], pnb[kMaxBeam], tot[kMaxBeam];
    int last[kMaxBeam], len[kMaxBeam];
    unsigned long long h[kMaxBeam], ph[kMaxBeam];
};

struct BeamGeom { int B, T, C, W, top, merge; };

// LM fusion (k_ctc_beam<T, true> only).  whole: the table sits in LDS (else one row per live beam is staged per frame); use_tab =
// alpha != 0 (alpha = 0: the table is never read and F = beta |prefix|).
struct LmGeom {
    const float *table;
    float *score;
    float alpha, beta;
    int order, eos, whole, use_tab;
};
// dynamic LDS of the LM variant: per beam set F and the label before `last`, the final scores and ranks, then the table or the rows
constexpr int kLmHeadWords = 2 * kMaxBeam * 2 + 2 * kMaxBeam;
size_t lm_lds_bytes(int C, int W, int order, bool whole, bool use_tab)
{
    size_t tab = C;                                    // alpha = 0: a row of C floats keeps any (unused) table read in bounds
    if (use_tab) {
        size_t rows = 1;
        for (int i = 1; i < order; ++i) rows *= (size_t)C;
        tab = whole ? rows * C : (size_t)W * C;
    }
    return (kLmHeadWords + tab) * sizeof(float);
}

// F of an extension: F(l + c) = F(l) + alpha log P(c | ctx(l)) + beta, one rounding order everywhere it is evaluated
__device__ __forceinline__ float lm_ext_bonus(float f, float lmv, float alpha, float beta) { return __fmaf_rn(alpha, lmv, f) + beta; }

template <typename T, bool LM>
__global__ void __launch_bounds__(BEAM_THREADS)
k_ctc_beam(const T *__restrict__ pred, const int *__restrict__ in_len, const BeamGeom g, const LmGeom lm, int *__restrict__ decoded,
           int *__restrict__ dlen, float *__restrict__ logp, int *__restrict__ hist)
{
    __shared__ BeamSet bs[2];
    __shared__ float s_pb[kMaxBeam], s_pnb[kMaxBeam], s_tot[kMaxBeam];       // stay candidates of the frame
    __shared__ unsigned emask[kMaxBeam * (kMaxClasses / 32)];                  // extension (slot, class) merged into an existing beam
    __shared__ float lps[kMaxClasses];
    __shared__ unsigned hcount[256];
    __shared__ unsigned long long l_key[kMaxBeam];
    __shared__ unsigned l_sec[kMaxBeam];
    __shared__ float l_score[kMaxBeam];
    __shared__ unsigned long long sel_prefix;
    __shared__ int sel_rem, sel_stop, sel_K, l_count, s_nb, s_plen[kMaxBeam];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = g.C, CP = C - 1, blank = C - 1, W = g.W;
    const int Tn = min(max(in_len[b], 0), g.T);
    const T *p = pred + (long long)b * g.T * C;
    int *hb = hist + (long long)b * g.T * W;

    // LM state (dynamic LDS): lF[set][slot], lp2[set][slot] (label before `last`, -1 if none), fin / perm (final re-rank), tab
    extern __shared__ float lm_dyn[];
    float *lF = lm_dyn;
    int *lp2 = reinterpret_cast<int *>(lm_dyn + 2 * kMaxBeam);
    float *fin = lm_dyn + 4 * kMaxBeam;
    int *perm = reinterpret_cast<int *>(lm_dyn + 5 * kMaxBeam);
    float *tab = lm_dyn + kLmHeadWords;
    const int V = C - 1;
    // row offset of beam k's context in `tab` (whole table) or of its staged row; ctx: bigram last, trigram last2 C + last, V = <s>
    auto lm_ctx = [&](int last, int p2) {
        const int l1 = last < 0 ? V : last, l2 = p2 < 0 ? V : p2;
        return lm.order == 1 ? 0 : (lm.order == 2 ? l1 : l2 * C + l1);
    };

    if (tid == 0) {
        bs[0].pb[0] = 0.f; bs[0].pnb[0] = -INFINITY; bs[0].tot[0] = 0.f;
        bs[0].last[0] = -1; bs[0].len[0] = 0; bs[0].h[0] = 0ull; bs[0].ph[0] = 0ull;
        s_nb = 1;
        if constexpr (LM) { lF[0] = 0.f; lp2[0] = -1; }
    }
    if constexpr (LM) {
        if (lm.use_tab && lm.whole) {
            int n = C;
            for (int i = 1; i < lm.order; ++i) n *= C;
            for (int i = tid; i < n; i += BEAM_THREADS) tab[i] = lm.table[i];
        }
    }
    float yv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        yv[q] = (Tn > 0 && c < C) ? to_f32(p[c]) : 0.f;
    }
    int cur = 0;
    __syncthreads();
    for (int t = 0; t < Tn; ++t) {
        // ---- 1. lp[c] = u[c] - logsumexp u of this frame, in every wave's registers (class lane + 64 q); the next frame is fetched
        float lpr[4];
        {
            float m = -INFINITY;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                lpr[q] = (lane + 64 * q < C) ? logf(yv[q] + kEps) : -INFINITY;
                m = fmaxf(m, lpr[q]);
            }
            m = wave_max(m);
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) s += (lane + 64 * q < C) ? expf(lpr[q] - m) : 0.f;
            const float lse = m + logf(wave_sum(s));
#pragma unroll
            for (int q = 0; q < 4; ++q) lpr[q] -= lse;
        }
        if (t + 1 < Tn) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = lane + 64 * q;
                if (c < C) yv[q] = to_f32(p[(long long)(t + 1) * C + c]);
            }
        }
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (lane + 64 * q < C) lps[lane + 64 * q] = lpr[q];
        }
        const BeamSet &S = bs[cur];
        BeamSet &N = bs[cur ^ 1];
        const int nb = s_nb;
        for (int i = tid; i < nb * (kMaxClasses / 32); i += BEAM_THREADS) emask[i] = 0u;
        if (tid == 0) l_count = 0;
        const float *cF = lF + cur * kMaxBeam;
        const int *cp2 = lp2 + cur * kMaxBeam;
        if constexpr (LM) {
            if (lm.use_tab && !lm.whole) {                 // stage the context row of every live beam: rows[k C + c]
                for (int k = wave; k < nb; k += BEAM_THREADS / 64) {
                    const float *src = lm.table + (long long)lm_ctx(S.last[k], cp2[k]) * C;
                    for (int c = lane; c < C; c += 64) tab[k * C + c] = src[c];
                }
            }
        }
        __syncthreads();

        // ---- 2./3. stay candidates, with the extension of the beam's parent merged in (if the parent is a beam)
        if (tid < nb) {
            const int m = tid;
            const int lastm = S.last[m], lenm = S.len[m];
            const float spb = S.tot[m] + lps[blank];
            float spnb = lenm > 0 ? S.pnb[m] + lps[lastm] : -INFINITY;
            if (lenm > 0) {
                const unsigned long long phm = S.ph[m];
                int par = -1;
#pragma unroll 8
                for (int k = 0; k < nb; ++k) par = (S.h[k] == phm && S.len[k] == lenm - 1) ? k : par;
                if (par >= 0) {
                    const float ext = (lastm == S.last[par] ? S.pb[par] : S.tot[par]) + lps[lastm];
                    spnb = lse2f(spnb, ext);
                    atomicOr(&emask[par * (kMaxClasses / 32) + (lastm >> 5)], 1u << (lastm & 31));
                }
            }
            s_pb[m] = spb; s_pnb[m] = spnb; s_tot[m] = lse2f(spb, spnb);
        }
        __syncthreads();

        // ---- 4./5. radix select of the best W candidates: 8-bit digits from the top of the 48-bit key; candidates recomputed per pass
        // visit(fn): fn(score, sec, acoustic) for every candidate of this thread with a finite score (score = acoustic without an LM)
        auto visit = [&](auto &&fn) {
            if (tid < nb) {
                const float s = s_tot[tid];
                if constexpr (LM) {
                    const float f = s + cF[tid];
                    if (f > -INFINITY) fn(f, (unsigned)tid << 8, s);
                } else {
                    if (s > -INFINITY) fn(s, (unsigned)tid << 8, s);
                }
            }
            for (int k = wave; k < nb; k += BEAM_THREADS / 64) {
                const float pbk = S.pb[k], totk = S.tot[k];
                const int lastk = S.last[k];
                float fk = 0.f;
                const float *row = tab;
                if constexpr (LM) {
                    fk = cF[k];
                    row = tab + (!lm.use_tab ? 0 : lm.whole ? lm_ctx(lastk, cp2[k]) * C : k * C);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = lane + 64 * q;
                    if (c < CP && !((emask[k * (kMaxClasses / 32) + (c >> 5)] >> (c & 31)) & 1u)) {
                        const float s = (c == lastk ? pbk : totk) + lpr[q];
                        if constexpr (LM) {
                            const float f = s + lm_ext_bonus(fk, lm.use_tab ? row[c] : 0.f, lm.alpha, lm.beta);
                            if (f > -INFINITY) fn(f, 0x8000u | ((unsigned)k << 8) | (unsigned)c, s);
                        } else {
                            if (s > -INFINITY) fn(s, 0x8000u | ((unsigned)k << 8) | (unsigned)c, s);
                        }
                    }
                }
            }
        };
        if (tid == 0) { sel_prefix = 0ull; sel_stop = 0; }
        for (int pass = 0; pass < 6; ++pass) {
            const int shift = 40 - 8 * pass;
            hcount[tid] = 0u;                          // BEAM_THREADS == 256 bins
            __syncthreads();
            if (sel_stop) break;                       // uniform: written before the barrier above
            const unsigned long long pre = sel_prefix >> (shift + 8);
            visit([&](float s, unsigned sec, float) {
                const unsigned long long key = cand_key(s, sec);
                if ((key >> (shift + 8)) == pre) atomicAdd(&hcount[(key >> shift) & 255u], 1u);
            });
            __syncthreads();
            if (wave == 0) {
                unsigned hb4[4], sl = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) { hb4[i] = hcount[4 * lane + i]; sl += hb4[i]; }
                unsigned suf = sl;                     // suffix sum over lanes >= lane
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_down(suf, d, 64);
                    if (lane + d < 64) suf += o;
                }
                int rem;
                if (pass == 0) {
                    const int total = (int)__shfl(suf, 0, 64);
                    if (total <= W) {                  // every candidate is kept
                        if (lane == 0) { sel_K = total; sel_stop = 1; sel_prefix = 0ull; }
                        rem = -1;
                    } else {
                        rem = W;
                        if (lane == 0) sel_K = W;
                    }
                } else {
                    rem = sel_rem;
                }
                if (rem > 0) {
                    const unsigned long long ok = __ballot(suf >= (unsigned)rem);
                    const int L = 63 - __clzll((long long)ok);
                    if (lane == L) {
                        unsigned above = suf - sl;
                        int v = 4 * L;
                        unsigned hv = hb4[0];
#pragma unroll
                        for (int i = 3; i >= 0; --i) {
                            if (above + hb4[i] >= (unsigned)rem) { v = 4 * L + i; hv = hb4[i]; break; }
                            above += hb4[i];
                        }
                        const int nrem = rem - (int)above;
                        sel_prefix |= (unsigned long long)v << shift;
                        sel_rem = nrem;
                        if ((int)hv == nrem) sel_stop = 1;    // the whole bin is taken: key >= prefix selects exactly K
                    }
                }
            }
            __syncthreads();
        }
        const unsigned long long thr = sel_prefix;
        const int K = sel_K;
        visit([&](float s, unsigned sec, float ac) {
            const unsigned long long key = cand_key(s, sec);
            if (key >= thr) {
                const int pos = atomicAdd(&l_count, 1);
                if (pos < kMaxBeam) { l_key[pos] = key; l_sec[pos] = sec; l_score[pos] = ac; }
            }
        });
        __syncthreads();

        // ---- 6. the kept candidates in rank order form the next beam; one history word each
        if (tid < K) {
            const unsigned long long my = l_key[tid];
            int r = 0;
            for (int j = 0; j < K; ++j) r += l_key[j] > my;
            const unsigned sec = l_sec[tid];
            const int k = (sec >> 8) & 127;
            const float s = l_score[tid];
            if (!(sec & 0x8000u)) {
                N.pb[r] = s_pb[k]; N.pnb[r] = s_pnb[k]; N.tot[r] = s;
                N.last[r] = S.last[k]; N.len[r] = S.len[k]; N.h[r] = S.h[k]; N.ph[r] = S.ph[k];
                hb[(long long)t * W + r] = k;
                if constexpr (LM) { lF[(cur ^ 1) * kMaxBeam + r] = cF[k]; lp2[(cur ^ 1) * kMaxBeam + r] = cp2[k]; }
            } else {
                const int c = sec & 255;
                N.pb[r] = -INFINITY; N.pnb[r] = s; N.tot[r] = s;
                N.last[r] = c; N.len[r] = S.len[k] + 1; N.h[r] = hmix(S.h[k], c); N.ph[r] = S.h[k];
                hb[(long long)t * W + r] = k | ((c + 1) << 16);
                if constexpr (LM) {
                    const float lmv = lm.use_tab ? tab[(!lm.use_tab ? 0 : lm.whole ? lm_ctx(S.last[k], cp2[k]) * C : k * C) + c] : 0.f;
                    lF[(cur ^ 1) * kMaxBeam + r] = lm_ext_bonus(cF[k], lmv, lm.alpha, lm.beta);
                    lp2[(cur ^ 1) * kMaxBeam + r] = S.last[k];
                }
            }
        }
        if (tid == 0) s_nb = K;
        cur ^= 1;
        __syncthreads();
    }

    // ---- backtrack the top paths through the history, merge repeats on request, pad with -1
    const BeamSet &F = bs[cur];
    const int nb = s_nb;
    if constexpr (LM) {
        // final S (+ alpha log P(</s> | prefix) with eos), then a counting rank over the nb beams; ties keep the lower slot first
        if (tid < nb) {
            float f = lF[cur * kMaxBeam + tid];
            if (lm.eos && lm.use_tab)
                f = __fmaf_rn(lm.alpha, lm.table[(long long)lm_ctx(F.last[tid], lp2[cur * kMaxBeam + tid]) * C + V], f);
            fin[tid] = F.tot[tid] + f;
        }
        __syncthreads();
        if (tid < nb) {
            const unsigned long long my = cand_key(fin[tid], (unsigned)tid);
            int r = 0;
            for (int j = 0; j < nb; ++j) r += cand_key(fin[j], (unsigned)j) > my;
            perm[r] = tid;
        }
        __syncthreads();
    }
    if (tid < g.top) {
        const int pth = tid;
        int *row = decoded + ((long long)pth * g.B + b) * g.T;
        int L = 0;
        float lp = -INFINITY, sc = -INFINITY;
        if (pth < nb) {
            const int src = LM ? perm[pth] : pth;
            L = F.len[src];
            lp = F.tot[src];
            if constexpr (LM) sc = fin[src];
            int s = src, pos = L;
            for (int tt = Tn - 1; tt >= 0 && pos > 0; --tt) {
                const int w = hb[(long long)tt * W + s];
                const int lab = (w >> 16) - 1;
                if (lab >= 0) row[--pos] = lab;
                s = min(w & 0xFFFF, W - 1);                  // (always < W: written by the rank step)
            }
            if (g.merge) {
                int n = 0, prev = -1;
                for (int i = 0; i < L; ++i) {
                    const int v = row[i];
                    if (v != prev) row[n++] = v;
                    prev = v;
                }
                L = n;
            }
        }
        s_plen[pth] = L;
        dlen[(long long)pth * g.B + b] = L;
        logp[(long long)b * g.top + pth] = lp;
        if constexpr (LM) lm.score[(long long)b * g.top + pth] = sc;
    }
    __syncthreads();
    for (int e = tid; e < g.top * g.T; e += BEAM_THREADS) {
        const int pth = e / g.T, i = e - pth * g.T;
        if (i >= s_plen[pth]) decoded[((long long)pth * g.B + b) * g.T + i] = -1;
    }
}

// ---- edit distance -----------------------------------------------------------------------------------------------------------------
// One wave per pair.  Lane l owns reference positions j = l E .. l E + E - 1 of the DP row (j = 0 .. R, R <= 64 E - 1).
template <int E>
__global__ void __launch_bounds__(64)
k_edit_distance(const int *__restrict__ hyp, int hs, const int *__restrict__ hl, const int *__restrict__ ref, int rs,
                const int *__restrict__ rl, const int *__restrict__ cmap, int classes, int *__restrict__ out, int *__restrict__ rlen_out)
{
    __shared__ int rc[64 * E];
    const int b = blockIdx.x, lane = threadIdx.x;
    constexpr int kBig = INT_MAX / 4;
    auto map = [&](int tok, bool &keep) {
        if (cmap && tok >= 0 && tok < classes) {
            tok = cmap[tok];
            keep = keep && tok >= 0;
        }
        return tok;
    };
    // reference: mapped, dropped tokens removed, compacted into LDS by ballot
    const int Rraw = min(max(rl[b], 0), rs);
    int R = 0;
    for (int i0 = 0; i0 < Rraw; i0 += 64) {
        const int i = i0 + lane;
        bool keep = i < Rraw;
        const int tok = map(keep ? ref[(long long)b * rs + i] : 0, keep);
        const unsigned long long mask = __ballot(keep);
        if (keep) rc[R + lanes_below(mask, lane)] = tok;
        R += __popcll(mask);
    }
    __syncthreads();
    int D[E], rt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = lane * E + e;
        D[e] = j;
        rt[e] = (j >= 1 && j <= R) ? rc[j - 1] : 0;
    }
    const int Hraw = min(max(hl[b], 0), hs);
    int i = 0;
    for (int h0 = 0; h0 < Hraw; h0 += 64) {
        bool keepv = h0 + lane < Hraw;
        const int tokv = map(keepv ? hyp[(long long)b * hs + h0 + lane] : 0, keepv);
        unsigned long long kmask = __ballot(keepv);
        while (kmask) {                                    // wave-uniform walk over the kept tokens
            const int src = __ffsll((long long)kmask) - 1;
            kmask &= kmask - 1ull;
            const int tok = __shfl(tokv, src, 64);
            ++i;
            const int left = __shfl_up(D[E - 1], 1, 64);   // D_prev[j - 1] of this lane's first position
            int tmp[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int j = lane * E + e;
                const int dl = e == 0 ? left : D[e - 1];
                tmp[e] = j == 0 ? i : min(D[e] + 1, dl + (rt[e] != tok ? 1 : 0));
            }
            int pm[E], s = kBig;
#pragma unroll
            for (int e = 0; e < E; ++e) { s = min(s, tmp[e] - (lane * E + e)); pm[e] = s; }
            int tot = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(tot, d, 64);
                if (lane >= d) tot = min(tot, o);
            }
            int excl = __shfl_up(tot, 1, 64);
            if (lane == 0) excl = kBig;
#pragma unroll
            for (int e = 0; e < E; ++e) D[e] = lane * E + e + min(excl, pm[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (lane * E + e == R) {
            out[b] = D[e];
            if (rlen_out) rlen_out[b] = R;
        }
}

}  // namespace

size_t ctc_beam_workspace_bytes(int B, int T, int W) { return (size_t)B * T * W * sizeof(int); }

int launch_ctc_greedy(int dtype, int B, int T, int C, const void *pred, const int *in_len, int *decoded, int *dlen, float *logp,
                      hipStream_t stream)
{
    if (C < 2 || C > kMaxClasses) return QK_ERR_UNSUPPORTED;
    if (!dtype_known(dtype)) return QK_ERR_INVALID_ARG;
    by_dtype(dtype, [&](auto t) {
        using TT = decltype(t);
        hipLaunchKernelGGL(k_ctc_greedy<TT>, dim3((unsigned)B), dim3(64), 0, stream, (const TT *)pred, in_len, B, T, C, decoded, dlen, logp);
    });
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

int launch_ctc_beam(int dtype, int B, int T, int C, const void *pred, const int *in_len, int W, int top, int merge, int *decoded,
                    int *dlen, float *logp, int *hist, hipStream_t stream)
{
    if (C < 2 || C > kMaxClasses || W < 1 || W > kMaxBeam || top < 1 || top > W) return QK_ERR_UNSUPPORTED;
    BeamGeom g;
    g.B = B; g.T = T; g.C = C; g.W = W; g.top = top; g.merge = merge ? 1 : 0;
    if (!dtype_known(dtype)) return QK_ERR_INVALID_ARG;
    LmGeom lm = {};
    by_dtype(dtype, [&](auto t) {
        using TT = decltype(t);
        hipLaunchKernelGGL((k_ctc_beam<TT, false>), dim3((unsigned)B), dim3(BEAM_THREADS), 0, stream, (const TT *)pred, in_len, g, lm, decoded,
                           dlen, logp, hist);
    });
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

int ctc_beam_lm_supported(int C, int W, int order)
{
    if (order < 1 || order > kMaxLmOrder || (order == 3 && C > kMaxLmTrigramClasses)) return 0;
    const bool whole = lm_lds_bytes(C, W, order, true, true) - kLmHeadWords * sizeof(float) <= kLmWholeTableBytes;
    return lm_lds_bytes(C, W, order, whole, true) <= kLmMaxDynLds;
}

int launch_ctc_beam_lm(int dtype, int B, int T, int C, const void *pred, const int *in_len, int W, int top, int merge, int order,
                       const float *table, float alpha, float beta, int eos, int *decoded, int *dlen, float *logp, float *score, int *hist,
                       hipStream_t stream)
{
    if (C < 2 || C > kMaxClasses || W < 1 || W > kMaxBeam || top < 1 || top > W || !ctc_beam_lm_supported(C, W, order))
        return QK_ERR_UNSUPPORTED;
    if (!dtype_known(dtype)) return QK_ERR_INVALID_ARG;
    BeamGeom g;
    g.B = B; g.T = T; g.C = C; g.W = W; g.top = top; g.merge = merge ? 1 : 0;
    LmGeom lm;
    lm.table = table; lm.score = score; lm.alpha = alpha; lm.beta = beta; lm.order = order; lm.eos = eos ? 1 : 0;
    lm.use_tab = alpha != 0.f;
    lm.whole = lm_lds_bytes(C, W, order, true, true) - kLmHeadWords * sizeof(float) <= kLmWholeTableBytes;
    const size_t lds = lm_lds_bytes(C, W, order, lm.whole, lm.use_tab);
    bool granted_ok = true;
    by_dtype(dtype, [&](auto t) {
        using TT = decltype(t);
        static std::atomic<int> granted[kMaxLdsDevices];
        granted_ok = lds <= 65536 || grant_dynamic_lds(reinterpret_cast<const void *>(&k_ctc_beam<TT, true>), lds, granted);
        if (granted_ok)
            hipLaunchKernelGGL((k_ctc_beam<TT, true>), dim3((unsigned)B), dim3(BEAM_THREADS), lds, stream, (const TT *)pred, in_len, g, lm,
                               decoded, dlen, logp, hist);
    });
    if (!granted_ok) return QK_ERR_LAUNCH;         // (HIP's error of the refusal is what the entry point reports)
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

int launch_edit_distance(int B, const int *hyp, int hs, const int *hl, const int *ref, int rs, const int *rl, const int *cmap,
                         int classes, int *out, int *rlen_out, hipStream_t stream)
{
    if (rs > kMaxEditRef) return QK_ERR_UNSUPPORTED;
    dim3 grid((unsigned)B), block(64);
#define QK_ED(E) hipLaunchKernelGGL(k_edit_distance<E>, grid, block, 0, stream, hyp, hs, hl, ref, rs, rl, cmap, classes, out, rlen_out)
    if (rs < 64) QK_ED(1);
    else if (rs < 128) QK_ED(2);
    else if (rs < 256) QK_ED(4);
    else if (rs < 512) QK_ED(8);
    else QK_ED(17);                                  // 64 x 17 = 1088 > 1024 + 1 positions
#undef QK_ED
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace qk
