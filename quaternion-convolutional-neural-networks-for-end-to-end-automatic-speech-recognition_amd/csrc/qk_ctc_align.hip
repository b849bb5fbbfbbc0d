// CTC forced alignment (include/qk.h, "CTC forced alignment"): the best path through the lattice of a KNOWN transcript.
//
// The lattice is the one k_ctc (qk_ctc.hip) sweeps twice with log-sum-exp; here it is swept ONCE with max-plus, and every cell keeps
// which predecessor won (2 bits: 0 = stay, 1 = from s - 1, 2 = from s - 2).  Same layout as k_ctc: one workgroup of 256 threads owns a
// sample, thread s owns state s of the extended sequence (blank, l1, blank, ..., lL, blank: S = 2 L + 1 <= 255 states), the previous
// frame's scores are double-buffered in LDS (one barrier per frame), the emission of the NEXT frame is fetched before the barrier.
//   * The choice of a predecessor does not depend on the per-frame normaliser, so the sweep runs on u = log(y + eps); the score is
//     formed afterwards from the path itself, sum_t (u[t][class of pi_t] - lse[t]), per thread over a fixed stride of frames, then in
//     the wave by xor-shuffles, then over the four waves in order: a fixed order, no atomics.
//   * Back-pointers: each wave packs its 64 with two ballots (low bits, high bits) and lane 0 stores the two 64-bit words -- 64 bytes
//     per frame and sample, no two lanes ever share a byte.  They live in LDS when the sample's frames fit (BPL) and in the caller's
//     workspace otherwise.
//   * LPS (as in k_ctc): the sample's (T, C) table of u fits in LDS as well and is built once with coalesced loads; otherwise every
//     emission is gathered from global memory one frame ahead of its use.
//   * One lane walks the back-pointers from the end state and leaves the state of every frame in LDS (one byte: S <= 255); path,
//     starts and ends are then written by all threads, the -1 fill included.
// Every LDS and global index is bounded by the clamped Tn, Ln and S, never by a raw input value: back-pointers are 0, 1 or 2 by
// construction and the backtrack clamps the state at 0 all the same.
#include "qk_ctc_lattice.h"
#include "qk_seq.h"

namespace qk {
namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr size_t kAlignLdsBudget = 150 * 1024;        // of the CU's 160 KB; above 64 KB the launcher asks for it explicitly

struct AlignGeom : LatticeGeom {};         // (its own name: the name is part of the kernels' symbols)

// LDS image, in this order (the 64-bit words first: they need 8-byte alignment):
//   bp[T][4 waves][2] u64 (BPL) | v[2][Smax] f32 | lse[T] f32 | cls[Smax] i32 | red[4] f32, flag[4] i32 | u[T][C] f32 (LPS) | state[T] u8
__host__ __device__ inline size_t align_bp_words(int T) { return (size_t)T * ALIGN_WAVES * 2; }
__host__ __device__ inline size_t align_lds_bytes(int T, int C, int Smax, bool lps, bool bpl)
{
    size_t n = bpl ? align_bp_words(T) * 8 : 0;
    n += (size_t)(2 * Smax + T + Smax + 8) * 4;
    if (lps) n += (size_t)T * C * 4;
    return n + (((size_t)T + 7) & ~(size_t)7);
}

template <typename T, bool LPS, bool BPL>
__global__ void __launch_bounds__(ALIGN_THREADS)
k_ctc_align(const T *__restrict__ pred, const int *__restrict__ labels, const int *__restrict__ in_len, const int *__restrict__ lab_len,
            int *__restrict__ path, int *__restrict__ starts, int *__restrict__ ends, float *__restrict__ score,
            unsigned long long *__restrict__ bp_ws, const AlignGeom g)
{
    extern __shared__ unsigned long long smem64[];
    unsigned long long *bp = BPL ? smem64 : bp_ws + (size_t)blockIdx.x * align_bp_words(g.T);
    float *vv = reinterpret_cast<float *>(smem64 + (BPL ? align_bp_words(g.T) : 0));
    float *lse = vv + 2 * g.Smax;
    int *cls_l = reinterpret_cast<int *>(lse + g.T);
    float *red = reinterpret_cast<float *>(cls_l + g.Smax);
    int *flag = reinterpret_cast<int *>(red + 4);
    float *lpt = red + 8;                                        // LPS: u[t][c]
    unsigned char *pst = reinterpret_cast<unsigned char *>(lpt + (LPS ? (size_t)g.T * g.C : 0));   // state of the path at frame t

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Tn = min(max(in_len[b], 0), g.T);
    const int Ln = min(max(lab_len[b], 0), g.Lmax);
    const int S = 2 * Ln + 1;
    const int blank = g.C - 1;
    const T *p = pred + (long long)b * g.T * g.C;
    int *prow = path + (long long)b * g.T;
    int *srow = starts + (long long)b * g.Lmax, *erow = ends + (long long)b * g.Lmax;
    // state of this thread (Smax <= ALIGN_THREADS is checked by the launcher); labels are clamped exactly as k_ctc clamps them
    const int s = tid;
    const bool live = s < S;
    const int lab_s = (live && (s & 1)) ? labels[b * g.Lmax + (s >> 1)] : 0;
    const int cls = (live && (s & 1)) ? min(max(lab_s, 0), g.C - 1) : blank;
    const bool skip_ok = live && (s & 1) && s >= 3 && lab_s != labels[b * g.Lmax + (s >> 1) - 1];      // s - 2 -> s
    if (s < g.Smax) cls_l[s] = cls;

    if (Tn == 0) {             // no frames: the empty labelling has the empty path, any other labelling has none
        for (int t = tid; t < g.T; t += ALIGN_THREADS) prow[t] = -1;
        for (int i = tid; i < g.Lmax; i += ALIGN_THREADS) { srow[i] = -1; erow[i] = -1; }
        if (tid == 0) score[b] = Ln == 0 ? 0.f : -INFINITY;
        return;
    }

    // ---- phase 0: u = log(p + eps) (LPS: into LDS, coalesced), per-frame normaliser lse[t] = logsumexp_c u[t][c] ------------------
    if constexpr (LPS) {
        for (int e = tid; e < Tn * g.C; e += ALIGN_THREADS) lpt[e] = __logf(to_f32(p[e]) + g.eps);
        __syncthreads();
    }
    for (int t = tid; t < Tn; t += ALIGN_THREADS) {
        float m = kNegInf;
        for (int c = 0; c < g.C; ++c) m = fmaxf(m, LPS ? lpt[t * g.C + c] : __logf(to_f32(p[t * g.C + c]) + g.eps));
        float sum = 0.f;
        for (int c = 0; c < g.C; ++c) sum += __expf((LPS ? lpt[t * g.C + c] : __logf(to_f32(p[t * g.C + c]) + g.eps)) - m);
        lse[t] = m + __logf(sum);
    }
    auto emit = [&](int t, int c) -> float {          // u[t][c], t < Tn, c < C
        if constexpr (LPS) return lpt[t * g.C + c];
        else return __logf(to_f32(p[t * g.C + c]) + g.eps);
    };

    // ---- phase 1: the max-plus sweep ------------------------------------------------------------------------------------------
    const bool wave_live = wave * 64 < S;              // a wave without a live state stores no back-pointers (none is ever read)
    float e_cur = live ? emit(0, cls) : 0.f;
    if (live) vv[s] = s < 2 ? e_cur : kNegInf;
    float e_next = (live && Tn > 1) ? emit(1, cls) : 0.f;
    __syncthreads();
    for (int t = 1; t < Tn; ++t) {
        const float *ap = vv + ((t - 1) & 1) * g.Smax;
        float *an = vv + (t & 1) * g.Smax;
        e_cur = e_next;
        if (live && t + 1 < Tn) e_next = emit(t + 1, cls);          // in flight across the barrier
        int back = 0;
        if (live) {
            float best = ap[s];                         // ties: stay, then s - 1, then s - 2 -- strict comparisons; -inf never wins
            if (s >= 1) { const float a1 = ap[s - 1]; if (a1 > best) { best = a1; back = 1; } }
            if (skip_ok) { const float a2 = ap[s - 2]; if (a2 > best) { best = a2; back = 2; } }
            an[s] = best <= kDead ? kNegInf : best + e_cur;
        }
        const unsigned long long lo = __ballot(back & 1), hi = __ballot(back >> 1);
        if (wave_live && lane == 0) {
            const size_t w = ((size_t)t * ALIGN_WAVES + wave) * 2;      // t < Tn <= T: inside bp[T][4][2]
            bp[w] = lo;
            bp[w + 1] = hi;
        }
        __syncthreads();
    }

    // ---- phase 2: end state and backtrack, one lane -------------------------------------------------------------------------------
    if (tid == 0) {
        const float *al = vv + ((Tn - 1) & 1) * g.Smax;
        int st = S - 1;
        float best = al[S - 1];
        if (S >= 2 && al[S - 2] > best) { best = al[S - 2]; st = S - 2; }        // S - 1 wins a tie
        const int feasible = best > kDead ? 1 : 0;
        if (feasible) {
            pst[Tn - 1] = (unsigned char)st;
            for (int t = Tn - 1; t >= 1; --t) {
                const size_t w = ((size_t)t * ALIGN_WAVES + (st >> 6)) * 2;      // st < S: a wave that stored frame t
                const int back = (int)((bp[w] >> (st & 63)) & 1) | ((int)((bp[w + 1] >> (st & 63)) & 1) << 1);
                st = max(st - back, 0);
                pst[t - 1] = (unsigned char)st;
            }
        }
        flag[0] = feasible;
    }
    __syncthreads();

    // ---- phase 3: the rows, by all threads ----------------------------------------------------------------------------------------
    if (!flag[0]) {            // no alignment fits (more labels, counting the blanks between repeats, than frames)
        for (int t = tid; t < g.T; t += ALIGN_THREADS) prow[t] = -1;
        for (int i = tid; i < g.Lmax; i += ALIGN_THREADS) { srow[i] = -1; erow[i] = -1; }
        if (tid == 0) score[b] = -INFINITY;
        return;
    }
    float part = 0.f;
    for (int t = tid; t < g.T; t += ALIGN_THREADS) {
        if (t >= Tn) { prow[t] = -1; continue; }
        const int st = min((int)pst[t], S - 1);
        const int c = cls_l[st];
        prow[t] = c;
        part += emit(t, c) - lse[t];
        if (st & 1) {          // a label state: (st >> 1) < Ln; its frames are contiguous, so each start / end is written once
            if (t == 0 || pst[t - 1] != pst[t]) srow[st >> 1] = t;
            if (t == Tn - 1 || pst[t + 1] != pst[t]) erow[st >> 1] = t + 1;
        }
    }
    for (int i = Ln + tid; i < g.Lmax; i += ALIGN_THREADS) { srow[i] = -1; erow[i] = -1; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) score[b] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One form of one element type.  1: the device refuses the LDS size, and the caller takes a form that needs less.
template <typename TT, bool LPS, bool BPL>
int launch_form(const void *pred, const int *labels, const int *in_len, const int *lab_len, int *path, int *starts, int *ends, float *score,
                void *ws, const AlignGeom &g, size_t lds, hipStream_t stream)
{
    static std::atomic<int> granted[kMaxLdsDevices];
    if (lds > 64 * 1024 && !grant_dynamic_lds(reinterpret_cast<const void *>(&k_ctc_align<TT, LPS, BPL>), lds, granted)) {
        (void)hipGetLastError();
        return 1;
    }
    hipLaunchKernelGGL((k_ctc_align<TT, LPS, BPL>), dim3((unsigned)g.B), dim3(ALIGN_THREADS), lds, stream, (const TT *)pred, labels, in_len,
                       lab_len, path, starts, ends, score, static_cast<unsigned long long *>(ws), g);
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace

size_t ctc_align_workspace_bytes(int B, int T) { return (size_t)B * align_bp_words(T) * 8; }      // the back-pointers of every frame

bool ctc_align_supported(int T, int C, int Lmax)
{
    return C <= ALIGN_THREADS && 2 * Lmax + 1 <= ALIGN_THREADS && align_lds_bytes(T, C, 2 * Lmax + 1, false, false) <= kAlignLdsBudget;
}

int launch_ctc_align(int dtype, int B, int T, int C, const void *pred, const int *labels, int Lmax, const int *in_len, const int *lab_len,
                     int *path, int *starts, int *ends, float *score, void *ws, hipStream_t stream)
{
    if (!ctc_align_supported(T, C, Lmax) || !dtype_known(dtype)) return QK_ERR_UNSUPPORTED;
    AlignGeom g;
    g.B = B; g.T = T; g.C = C; g.Lmax = Lmax; g.Smax = 2 * Lmax + 1; g.eps = 1e-7f;
    // forms in order of preference: back-pointers and table in LDS, back-pointers only, table only, neither
    static const bool kForms[4][2] = {{true, true}, {false, true}, {true, false}, {false, false}};      // {lps, bpl}
    size_t budget = kAlignLdsBudget;
    for (int f = 0; f < 4; ++f) {
        const bool lps = kForms[f][0], bpl = kForms[f][1];
        const size_t lds = align_lds_bytes(T, C, g.Smax, lps, bpl);
        if (lds > budget) continue;
        int rc = 0;
        by_dtype(dtype, [&](auto t) {
            using TT = decltype(t);
            static constexpr decltype(&launch_form<TT, true, true>) kLaunch[2][2] = {      // [lps][bpl]
                {&launch_form<TT, false, false>, &launch_form<TT, false, true>}, {&launch_form<TT, true, false>, &launch_form<TT, true, true>}};
            rc = kLaunch[lps][bpl](pred, labels, in_len, lab_len, path, starts, ends, score, ws, g, lds, stream);
        });
        if (rc != 1) return rc;
        budget = 64 * 1024;                    // the device grants no more than the default: a smaller form of the same kernel
    }
    return QK_ERR_UNSUPPORTED;
}

}  // namespace qk
