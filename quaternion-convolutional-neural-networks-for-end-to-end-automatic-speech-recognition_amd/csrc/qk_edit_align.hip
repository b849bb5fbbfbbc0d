// Scoring alignment (include/qk.h, "Scoring alignment"): the Levenshtein alignment of a hypothesis to a reference under a fixed tie
// rule -- correct / substitution / deletion / insertion counts, the aligned pairs, the confusion matrix.
//
// The row sweep is k_edit_distance's (qk_ctc_decode.hip), copied, not shared: one wave per pair, lane l owns the E consecutive reference
// positions j = l E .. l E + E - 1 of the DP row (j = 0 .. R <= 64 E - 1), the chain of horizontal steps inside a row is resolved by a
// min-plus prefix scan (in-lane, then six shuffles), after which D[i][.] is exact.
//   * Decisions.  With D[i][.] exact every lane holds the three candidates of its cells in registers and forms the 2-bit decision by
//     EQUALITY against D[i][j], in the priority of the definition: 0 = diagonal if D[i][j] == D[i-1][j-1] + (h_i != r_j), else
//     1 = deletion if D[i][j] == D[i][j-1] + 1, else 2 = insertion.  Column 0 is always an insertion.
//   * Packing.  For each e the wave takes two ballots (low bit, high bit): bit l of the pair is the decision of cell j = l E + e.  Lane
//     e stores the pair of its e, so row i is E x 16 bytes = exactly 2 bits per cell and no two lanes ever share a word.
//   * Storage.  table[H][E][2] u64 lives in LDS when the pair's STRIDES (not its lengths) say the whole LDS image fits in 64 KB (TBL),
//     and in the caller's workspace otherwise; edit_align_table_in_lds() is the one rule, used by the launcher and by the workspace size.
//   * Backtrack.  Lane 0 walks from (H, R) to (0, 0), at most H + R steps, and leaves the operations in reverse order in LDS (reference
//     token, hypothesis token, operation); it also counts C / S / D / I.  All lanes then write the forward-ordered rows with their -1
//     tails, and add their pairs to the confusion matrix with integer atomicAdd (order-independent).
// Every LDS and global index is bounded by the clamped lengths H <= hs, R <= rs and by A = hs + rs, never by a token value: a token
// indexes the matrix only after the check 0 <= token < K, and class_map only after 0 <= token < classes.
#include "qk_common.h"

namespace qk {
namespace {

constexpr int kMaxAlignSeq = 1024;
constexpr size_t kEditAlignLdsBudget = 64 * 1024;

__host__ __device__ inline int edit_align_e(int rs) { return rs < 64 ? 1 : rs < 128 ? 2 : rs < 256 ? 4 : rs < 512 ? 8 : 17; }
__host__ __device__ inline size_t edit_align_table_words(int hs, int E) { return (size_t)hs * E * 2; }      // u64 words of one pair
// LDS image, in this order (the 64-bit words first):
//   table[hs][E][2] u64 (TBL) | rc[64 E] i32 | hc[hs] i32 | rev_ref[A] i32 | rev_hyp[A] i32 | misc[8] i32 | rev_op[A] u8
__host__ __device__ inline size_t edit_align_lds_bytes(int hs, int rs, bool tbl)
{
    const int E = edit_align_e(rs), A = hs + rs;
    size_t n = tbl ? edit_align_table_words(hs, E) * 8 : 0;
    n += (size_t)(64 * E + hs + 2 * A + 8) * 4;
    return n + (((size_t)A + 7) & ~(size_t)7);
}

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

template <int E, bool TBL>
__global__ void __launch_bounds__(64)
k_edit_align(const int *__restrict__ hyp, int hs, const int *__restrict__ hl, const int *__restrict__ ref, int rs,
             const int *__restrict__ rl, const int *__restrict__ cmap, int classes, int *__restrict__ counts, int *__restrict__ ali_ref,
             int *__restrict__ ali_hyp, int *__restrict__ ali_len, int *__restrict__ conf, int K, unsigned long long *tab_ws)
{
    extern __shared__ unsigned long long smem64[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int A = hs + rs;
    unsigned long long *tab = TBL ? smem64 : tab_ws + (size_t)b * edit_align_table_words(hs, E);
    int *rc = reinterpret_cast<int *>(smem64 + (TBL ? edit_align_table_words(hs, E) : 0));
    int *hc = rc + 64 * E;
    int *rev_ref = hc + hs;
    int *rev_hyp = rev_ref + A;
    int *misc = rev_hyp + A;                                       // n, C, S, D, I
    unsigned char *rev_op = reinterpret_cast<unsigned char *>(misc + 8);
    constexpr int kBig = INT_MAX / 4;
    auto map = [&](int tok, bool &keep) {
        if (cmap && tok >= 0 && tok < classes) {
            tok = cmap[tok];
            keep = keep && tok >= 0;
        }
        return tok;
    };
    // both sequences: mapped, dropped tokens removed, compacted into LDS by ballot
    auto compact = [&](const int *seq, int stride, int n_raw, int *dst) {
        int n = 0;
        for (int i0 = 0; i0 < n_raw; i0 += 64) {
            const int i = i0 + lane;
            bool keep = i < n_raw;
            const int tok = map(keep ? seq[(long long)b * stride + i] : 0, keep);
            const unsigned long long mask = __ballot(keep);
            if (keep) dst[n + lanes_below(mask, lane)] = tok;      // n + ... < n_raw <= stride
            n += __popcll(mask);
        }
        return n;
    };
    const int R = compact(ref, rs, min(max(rl[b], 0), rs), rc);
    const int H = compact(hyp, hs, min(max(hl[b], 0), hs), hc);
    __syncthreads();

    // ---- the row sweep with decisions ---------------------------------------------------------------------------------------------
    int D[E], rt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = lane * E + e;
        D[e] = j;
        rt[e] = (j >= 1 && j <= R) ? rc[j - 1] : 0;
    }
    for (int i = 1; i <= H; ++i) {
        const int tok = hc[i - 1];
        const int left = __shfl_up(D[E - 1], 1, 64);       // D[i-1][j-1] of this lane's first position
        int dg[E], tmp[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = lane * E + e;
            dg[e] = (e == 0 ? left : D[e - 1]) + (rt[e] != tok ? 1 : 0);
            tmp[e] = j == 0 ? i : min(D[e] + 1, dg[e]);
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
        for (int e = 0; e < E; ++e) D[e] = lane * E + e + min(excl, pm[e]);       // D[i][j], exact
        const int nleft = __shfl_up(D[E - 1], 1, 64);      // D[i][j-1] of this lane's first position
        unsigned long long mylo = 0, myhi = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = lane * E + e;
            const int dl = e == 0 ? nleft : D[e - 1];
            const int code = j == 0 ? 2 : D[e] == dg[e] ? 0 : D[e] == dl + 1 ? 1 : 2;
            const unsigned long long lo = __ballot(code & 1), hi = __ballot(code >> 1);
            if (lane == e) { mylo = lo; myhi = hi; }
        }
        if (lane < E) {                                    // i - 1 < H <= hs: inside table[hs][E][2]
            const size_t w = ((size_t)(i - 1) * E + lane) * 2;
            tab[w] = mylo;
            tab[w + 1] = myhi;
        }
    }
    __syncthreads();

    // ---- backtrack, one lane: at most H + R steps ----------------------------------------------------------------------------------
    if (lane == 0) {
        int i = H, j = R, n = 0, nc = 0, ns = 0, nd = 0, ni = 0;
        while ((i > 0 || j > 0) && n < A) {
            int code;
            if (i == 0) code = 1;
            else if (j == 0) code = 2;
            else {
                const size_t w = ((size_t)(i - 1) * E + j % E) * 2;
                const int l = j / E;                       // j <= R <= 64 E - 1: l < 64
                code = (int)((tab[w] >> l) & 1) | ((int)((tab[w + 1] >> l) & 1) << 1);
            }
            if (code == 0) {
                const int r = rc[j - 1], h = hc[i - 1];
                rev_ref[n] = r; rev_hyp[n] = h; rev_op[n] = 0;
                if (r == h) ++nc; else ++ns;
                --i; --j;
            } else if (code == 1) {
                rev_ref[n] = rc[j - 1]; rev_hyp[n] = -1; rev_op[n] = 1;
                ++nd; --j;
            } else {
                rev_ref[n] = -1; rev_hyp[n] = hc[i - 1]; rev_op[n] = 2;
                ++ni; --i;
            }
            ++n;
        }
        misc[0] = n; misc[1] = nc; misc[2] = ns; misc[3] = nd; misc[4] = ni;
    }
    __syncthreads();

    // ---- outputs, by all lanes -----------------------------------------------------------------------------------------------------
    const int n = misc[0];
    if (lane < 4) counts[(long long)b * 4 + lane] = misc[1 + lane];
    if (ali_ref) {
        if (lane == 0) ali_len[b] = n;
        for (int k = lane; k < A; k += 64) {
            const bool in = k < n;
            ali_ref[(long long)b * A + k] = in ? rev_ref[n - 1 - k] : -1;
            ali_hyp[(long long)b * A + k] = in ? rev_hyp[n - 1 - k] : -1;
        }
    }
    if (conf) {
        for (int k = lane; k < n; k += 64) {
            const int op = rev_op[k], r = rev_ref[k], h = rev_hyp[k];
            const bool r_in = r >= 0 && r < K, h_in = h >= 0 && h < K;
            if (op == 0) { if (r_in && h_in) atomicAdd(conf + r * (K + 1) + h, 1); }
            else if (op == 1) { if (r_in) atomicAdd(conf + r * (K + 1) + K, 1); }
            else if (h_in) atomicAdd(conf + K * (K + 1) + h, 1);
        }
    }
}

template <int E>
int launch_e(bool tbl, size_t lds, int B, const int *hyp, int hs, const int *hl, const int *ref, int rs, const int *rl, const int *cmap,
             int classes, int *counts, int *ali_ref, int *ali_hyp, int *ali_len, int *conf, int K, void *ws, hipStream_t stream)
{
    dim3 grid((unsigned)B), block(64);
    if (tbl)
        hipLaunchKernelGGL((k_edit_align<E, true>), grid, block, lds, stream, hyp, hs, hl, ref, rs, rl, cmap, classes, counts, ali_ref, ali_hyp,
                           ali_len, conf, K, static_cast<unsigned long long *>(ws));
    else
        hipLaunchKernelGGL((k_edit_align<E, false>), grid, block, lds, stream, hyp, hs, hl, ref, rs, rl, cmap, classes, counts, ali_ref, ali_hyp,
                           ali_len, conf, K, static_cast<unsigned long long *>(ws));
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace

bool edit_align_table_in_lds(int hs, int rs) { return edit_align_lds_bytes(hs, rs, true) <= kEditAlignLdsBudget; }

size_t edit_align_workspace_bytes(int B, int hs, int rs)
{
    return edit_align_table_in_lds(hs, rs) ? 0 : (size_t)B * edit_align_table_words(hs, edit_align_e(rs)) * 8;
}

int launch_edit_align(int B, const int *hyp, int hs, const int *hl, const int *ref, int rs, const int *rl, const int *cmap, int classes,
                      int *counts, int *ali_ref, int *ali_hyp, int *ali_len, int *conf, int K, void *ws, hipStream_t stream)
{
    if (hs > kMaxAlignSeq || rs > kMaxAlignSeq) return QK_ERR_UNSUPPORTED;
    const bool tbl = edit_align_table_in_lds(hs, rs);
    const size_t lds = edit_align_lds_bytes(hs, rs, tbl);
    if (lds > kEditAlignLdsBudget) return QK_ERR_UNSUPPORTED;
#define QK_EA(E) return launch_e<E>(tbl, lds, B, hyp, hs, hl, ref, rs, rl, cmap, classes, counts, ali_ref, ali_hyp, ali_len, conf, K, ws, stream)
    switch (edit_align_e(rs)) {
    case 1: QK_EA(1);
    case 2: QK_EA(2);
    case 4: QK_EA(4);
    case 8: QK_EA(8);
    default: QK_EA(17);                              // 64 x 17 = 1088 > 1024 + 1 positions
    }
#undef QK_EA
}

}  // namespace qk
