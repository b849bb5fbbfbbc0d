// Device-resident corpus (include/qk_data.h): one launch gathers a batch of packed int16 utterances, their labels and aux words into
// padded matrices, at the row of the schedule that a keyed permutation of the device cursor names.
// A pure copy, HBM-bound: batch * n_out * 2 bytes are written and the utterances' bytes are read.  Source rows start on 16-byte
// boundaries, destination row b starts b * n_out * 2 bytes into wave_out, so the two are mutually misaligned by any even byte count:
// the body of a row is written with ALIGNED 16-byte stores, each fed by the two aligned 16-byte loads that cover it and a funnel by the
// row's (workgroup-uniform) shift; the up to 7 + 7 elements in front of and behind the body are written element by element.
#include "qk_common.h"

#include "../../include/qk_data.h"

namespace qk {
namespace {

constexpr int kThreads = 256;
constexpr int kVecPerThread = 4;
constexpr int kVecPerBlock = kThreads * kVecPerThread;       // 16-byte stores of one wave-part workgroup: 16 KiB of one row

__host__ __device__ inline uint32_t fmix(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// perm of qk_data.h: written ONCE, evaluated by qk_epoch_permutation on the host and by every workgroup of the kernel
__host__ __device__ inline uint32_t perm_row(uint32_t seed, uint32_t epoch, uint32_t pos, uint32_t nb)
{
    uint32_t k = 2;
    while (k < 32 && (1ull << k) < nb) k += 2;
    const uint32_t half = k / 2, mask = (1u << half) - 1u;
    const uint32_t key = fmix(seed + 0x9E3779B1u * epoch);
    const unsigned long long bound = 1ull << k;
    uint32_t x = pos;
    for (unsigned long long pass = 0; pass < bound; ++pass) {
        uint32_t l = x >> half, r = x & mask;
        for (uint32_t round = 0; round < 4; ++round) {
            const uint32_t t = l ^ (fmix(key ^ (r * 0x9E3779B1u + round * 0x7F4A7C15u + 0x165667B1u)) & mask);
            l = r;
            r = t;
        }
        x = (l << half) | r;
        if (x < nb) return x;
    }
    return pos;                                              // (unreachable: a cycle of a bijection on 2^k points is no longer)
}

struct Plan { uint32_t p, epoch, pos, row; };

__device__ inline Plan plan_of(const qk_batch_schedule_t &sc, uint32_t position, const uint32_t *__restrict__ cursor)
{
    Plan pl;
    const uint32_t nb = (uint32_t)sc.num_batches;
    pl.p = cursor ? *cursor : position;
    pl.epoch = pl.p / nb;
    pl.pos = pl.p - pl.epoch * nb;
    pl.row = sc.shuffle ? perm_row(sc.seed, pl.epoch, pl.pos, nb) : pl.pos;
    return pl;
}

// utterance of slot b, or -1 for an empty slot
__device__ inline int slot_utt(const qk_corpus_t &c, const qk_batch_schedule_t &sc, uint32_t row, int b)
{
    const int u = sc.batches[(size_t)row * (size_t)sc.batch + (size_t)b];
    return (u < 0 || u >= c.num_utts) ? -1 : u;
}

// samples of utterance u that reach the output (0 for an empty slot or a span that is not inside the pack) and where they start
__device__ inline int wave_span(const qk_corpus_t &c, int u, int n_out, const int16_t **src)
{
    *src = c.wave_pack;
    if (u < 0) return 0;
    const long long len = c.wave_len[u], off = c.wave_off[u];
    if (len <= 0 || off < 0 || (off & 7) || off > c.wave_samples || ((len + 7) & ~7ll) > c.wave_samples - off) return 0;
    *src = c.wave_pack + off;
    return (int)(len < n_out ? len : n_out);
}

__device__ inline int label_span(const qk_corpus_t &c, int u, int l_out, long long *off_out)
{
    *off_out = 0;
    if (u < 0) return 0;
    const long long len = c.label_len[u], off = c.label_off[u];
    if (len <= 0 || off < 0 || off > c.label_words || len > c.label_words - off) return 0;
    *off_out = off;
    return (int)(len < l_out ? len : l_out);
}

// the 8 elements that start S elements into the 16 elements {a, b}
template <int S>
__device__ __forceinline__ uint4 funnel(const uint4 &a, const uint4 &b)
{
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    constexpr int q = S >> 1;
    if constexpr (S & 1)
        return make_uint4((w[q] >> 16) | (w[q + 1] << 16), (w[q + 1] >> 16) | (w[q + 2] << 16), (w[q + 2] >> 16) | (w[q + 3] << 16),
                          (w[q + 3] >> 16) | (w[q + 4] << 16));
    else
        return make_uint4(w[q], w[q + 1], w[q + 2], w[q + 3]);
}

// keep the first m (< 8) elements of a group, zero the rest
__device__ __forceinline__ uint4 keep_first(const uint4 &v, int m)
{
    const auto word = [m](uint32_t w, int k) { return w & ((2 * k < m ? 0xFFFFu : 0u) | (2 * k + 1 < m ? 0xFFFF0000u : 0u)); };
    return make_uint4(word(v.x, 0), word(v.y, 1), word(v.z, 2), word(v.w, 3));
}

// The part of a row's body that one workgroup writes: 16-byte groups [v0 + i * kThreads] below v_end.  Group v holds row elements
// head + 8 v ..: S = head elements into the aligned source group 8 v.
template <int S>
__device__ __forceinline__ void copy_body(const int16_t *__restrict__ src, int16_t *__restrict__ dst, int n, int v0, int v_end)
{
    uint4 ga[kVecPerThread], gb[kVecPerThread];
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
        const int v = v0 + i * kThreads, a0 = 8 * v;
        ga[i] = gb[i] = make_uint4(0u, 0u, 0u, 0u);
        if (v < v_end && a0 < n) ga[i] = *reinterpret_cast<const uint4 *>(src + a0);
        if (S != 0 && v < v_end && a0 + 8 < n) gb[i] = *reinterpret_cast<const uint4 *>(src + a0 + 8);
    }
#pragma unroll
    for (int i = 0; i < kVecPerThread; ++i) {
        const int v = v0 + i * kThreads;
        if (v < v_end) {
            const int j0 = S + 8 * v, m = n - j0;           // m: elements of the group that are samples
            uint4 o = funnel<S>(ga[i], gb[i]);
            if (m < 8) o = m > 0 ? keep_first(o, m) : make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4 *>(dst + j0) = o;
        }
    }
}

// Workgroups [0, batch * chunks): 16 KiB of the body of one row of wave_out each (chunk 0 also writes the row's head and tail).
// Workgroups behind them: 256 elements of labels_out / aux_out each, and with them the per-slot words and the plan.
__global__ void __launch_bounds__(kThreads)
k_corpus_batch(qk_corpus_t c, qk_batch_schedule_t sc, uint32_t position, const uint32_t *__restrict__ cursor, int n_out, int l_out,
               int chunks, int16_t *__restrict__ wave_out, int *__restrict__ lengths_out, int *__restrict__ labels_out,
               int *__restrict__ label_length_out, int *__restrict__ aux_out, int *__restrict__ utt_out, int *__restrict__ plan)
{
    const Plan pl = plan_of(sc, position, cursor);
    const int tid = (int)threadIdx.x;
    const unsigned wave_blocks = (unsigned)sc.batch * (unsigned)chunks;
    if (blockIdx.x < wave_blocks) {
        const int b = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)chunks);
        const int16_t *src;
        const int n = wave_span(c, slot_utt(c, sc, pl.row, b), n_out, &src);
        int16_t *dst = wave_out + (size_t)b * (size_t)n_out;
        int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 1;     // elements in front of the first 16-byte boundary
        if (head > n_out) head = n_out;
        const int nv = (n_out - head) >> 3;                 // aligned 16-byte groups of the row
        const int v_end = min(nv, (chunk + 1) * kVecPerBlock);
        const int v0 = chunk * kVecPerBlock + tid;
        if (v0 - tid < v_end) {
            switch (head) {                                  // (the same in every thread of the workgroup; nv > 0: head < 8)
            case 0: copy_body<0>(src, dst, n, v0, v_end); break;
            case 1: copy_body<1>(src, dst, n, v0, v_end); break;
            case 2: copy_body<2>(src, dst, n, v0, v_end); break;
            case 3: copy_body<3>(src, dst, n, v0, v_end); break;
            case 4: copy_body<4>(src, dst, n, v0, v_end); break;
            case 5: copy_body<5>(src, dst, n, v0, v_end); break;
            case 6: copy_body<6>(src, dst, n, v0, v_end); break;
            case 7: copy_body<7>(src, dst, n, v0, v_end); break;
            default: break;
            }
        }
        if (chunk == 0 && tid < 16) {                        // threads 0-7: the head; threads 8-15: the tail
            const int j = tid < 8 ? tid : head + 8 * nv + (tid - 8);
            const bool mine = tid < 8 ? tid < head : j < n_out;
            if (mine) dst[j] = j < n ? src[j] : (int16_t)0;
        }
        return;
    }
    const long long i = (long long)(blockIdx.x - wave_blocks) * kThreads + tid;
    if (i >= (long long)sc.batch * l_out) return;
    const int b = (int)(i / l_out), j = (int)(i - (long long)b * l_out);
    const int u = slot_utt(c, sc, pl.row, b);
    long long off;
    const int l = label_span(c, u, l_out, &off);
    labels_out[i] = j < l ? c.label_pack[off + j] : 0;
    if (aux_out) aux_out[i] = j < l ? c.aux_pack[off + j] : -1;
    if (j == 0) {                                            // l_out >= 1: every slot has exactly one element 0
        const int16_t *src;
        lengths_out[b] = wave_span(c, u, n_out, &src);
        label_length_out[b] = l;
        if (utt_out) utt_out[b] = u;
    }
    if (i == 0 && plan) {
        plan[0] = (int)pl.p; plan[1] = (int)pl.epoch; plan[2] = (int)pl.pos; plan[3] = (int)pl.row;
    }
}

bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_epoch_permutation(uint32_t seed, uint32_t epoch, int32_t num_batches, int32_t *out_host)
{
    if (num_batches < 1) { set_error("qk_epoch_permutation: num_batches must be >= 1 (got %d)", num_batches); return QK_ERR_INVALID_ARG; }
    if (!out_host) { set_error("qk_epoch_permutation: NULL out_host"); return QK_ERR_INVALID_ARG; }
    for (int32_t pos = 0; pos < num_batches; ++pos) out_host[pos] = (int32_t)perm_row(seed, epoch, (uint32_t)pos, (uint32_t)num_batches);
    return QK_OK;
}

int qk_corpus_batch(const qk_corpus_t *corpus, const qk_batch_schedule_t *schedule, uint32_t position, const uint32_t *cursor_dev,
                    int32_t n_out, int32_t l_out, int16_t *wave_out, int32_t *lengths_out, int32_t *labels_out,
                    int32_t *label_length_out, int32_t *aux_out, int32_t *utt_out, int32_t *plan, void *stream)
{
    const char *what = "qk_corpus_batch";
    if (!corpus || !schedule) { set_error("%s: NULL corpus or schedule", what); return QK_ERR_INVALID_ARG; }
    const qk_corpus_t &c = *corpus;
    const qk_batch_schedule_t &sc = *schedule;
    if (!c.wave_pack || !c.wave_off || !c.wave_len || !c.label_pack || !c.label_off || !c.label_len || !sc.batches) {
        set_error("%s: NULL corpus array or NULL batches", what);
        return QK_ERR_INVALID_ARG;
    }
    if (!wave_out || !lengths_out || !labels_out || !label_length_out) { set_error("%s: NULL output", what); return QK_ERR_INVALID_ARG; }
    if (aux_out && !c.aux_pack) { set_error("%s: aux_out given, but the corpus has no aux_pack", what); return QK_ERR_INVALID_ARG; }
    if (sc.batch < 1 || sc.num_batches < 1) { set_error("%s: batch and num_batches must be >= 1 (got %d, %d)", what, sc.batch, sc.num_batches); return QK_ERR_INVALID_ARG; }
    if (n_out < 1 || l_out < 1) { set_error("%s: n_out and l_out must be >= 1 (got %d, %d)", what, n_out, l_out); return QK_ERR_INVALID_ARG; }
    if (c.num_utts < 0 || c.wave_samples < 0 || c.label_words < 0) {
        set_error("%s: num_utts, wave_samples and label_words must be >= 0 (got %d, %lld, %lld)", what, c.num_utts, (long long)c.wave_samples, (long long)c.label_words);
        return QK_ERR_INVALID_ARG;
    }
    if (sc.shuffle != 0 && sc.shuffle != 1) { set_error("%s: shuffle must be 0 or 1 (got %d)", what, sc.shuffle); return QK_ERR_INVALID_ARG; }
    if (!aligned_to(c.wave_pack, 16) || !aligned_to(wave_out, 2) || !aligned_to(c.wave_off, 8) || !aligned_to(c.label_off, 8)
        || !aligned_to(c.wave_len, 4) || !aligned_to(c.label_pack, 4) || !aligned_to(c.label_len, 4) || !aligned_to(c.aux_pack, 4)
        || !aligned_to(sc.batches, 4) || !aligned_to(cursor_dev, 4) || !aligned_to(lengths_out, 4) || !aligned_to(labels_out, 4)
        || !aligned_to(label_length_out, 4) || !aligned_to(aux_out, 4) || !aligned_to(utt_out, 4) || !aligned_to(plan, 4)) {
        set_error("%s: alignment: wave_pack needs 16 bytes, every other array its element size", what);
        return QK_ERR_INVALID_ARG;
    }
    if ((long long)sc.batch * n_out >= (1ll << 31) || (long long)sc.batch * l_out >= (1ll << 31)) {
        set_error("%s: an output of 2^31 elements or more is not supported (batch %d, n_out %d, l_out %d)", what, sc.batch, n_out, l_out);
        return QK_ERR_UNSUPPORTED;
    }
    const int groups = n_out / 8;
    const int chunks = groups > kVecPerBlock ? (groups + kVecPerBlock - 1) / kVecPerBlock : 1;
    const long long label_blocks = ((long long)sc.batch * l_out + kThreads - 1) / kThreads;
    const long long blocks = (long long)sc.batch * chunks + label_blocks;
    if (blocks >= (1ll << 31)) { set_error("%s: batch %d needs more workgroups than one launch has", what, sc.batch); return QK_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(k_corpus_batch, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, c, sc, position, cursor_dev,
                       (int)n_out, (int)l_out, chunks, wave_out, lengths_out, labels_out, label_length_out, aux_out, utt_out, plan);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return QK_OK;
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return QK_ERR_LAUNCH;
}

}  // extern "C"
