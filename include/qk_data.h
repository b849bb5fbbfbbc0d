/* Device-resident corpus: epoch shuffling and batch assembly on the device -- the entry points of the data side, exported by the
 * same libqk_hip.so behind version 103 of include/qk.h (a third header and a third table, as include/qk_opt.h is the second).
 *
 * A training step that is one captured graph needs a batch that is new on every replay without a launch argument that depends on
 * the step.  The corpus therefore lives in device memory, packed once; a batch is named by a POSITION in an endless sequence of
 * epochs, read from a device cursor; the order of an epoch is a keyed permutation of the schedule's rows evaluated by the kernel,
 * and by the host from the same function, so the host knows every draw without reading anything back. */
#ifndef QK_DATA_H_
#define QK_DATA_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The corpus: HOST struct of DEVICE arrays, built once.
 *
 *   wave_pack   int16, wave_samples of them, 16-byte aligned.  Utterance u occupies [wave_off[u], wave_off[u] + wave_len[u]).
 *   wave_off    int64 (num_utts): every offset is a multiple of 8 samples (16 bytes); the gaps are zero; the pack reaches at least
 *               to wave_off[u] + wave_len[u] rounded up to a multiple of 8, for every u.
 *   wave_len    int32 (num_utts), may be 0.
 *   label_pack  int32, label_words of them; utterance u's labels occupy [label_off[u], label_off[u] + label_len[u]).
 *   label_off   int64 (num_utts), label_len int32 (num_utts), may be 0.
 *   aux_pack    int32, label_words of them, or NULL: one word per label under the label offsets (the hand-labelled start samples).
 *
 * An utterance whose length is negative, whose offset is negative or (waveforms) not a multiple of 8, or whose span leaves its
 * pack is read as EMPTY (length 0), never dereferenced. */
typedef struct qk_corpus_t {
    const int16_t *wave_pack;
    const int64_t *wave_off;
    const int32_t *wave_len;
    const int32_t *label_pack;
    const int64_t *label_off;
    const int32_t *label_len;
    const int32_t *aux_pack;     /* optional */
    int64_t wave_samples;        /* samples in wave_pack, a multiple of 8 */
    int64_t label_words;         /* words in label_pack (and in aux_pack) */
    int32_t num_utts;
    int32_t reserved;            /* 0 */
} qk_corpus_t;

/* The schedule: HOST struct.  batches is a DEVICE (num_batches, batch) int32 matrix of utterance indices; an index < 0 or
 * >= num_utts is an EMPTY SLOT.  Data-parallel ranks use disjoint `batches` (and may share seed: the permutation is over rows). */
typedef struct qk_batch_schedule_t {
    const int32_t *batches;
    int32_t num_batches;
    int32_t batch;
    uint32_t seed;
    int32_t shuffle;             /* 0 or 1 */
} qk_batch_schedule_t;

#define QK_CORPUS_PLAN_WORDS 4

/* One batch, as ONE launch: no workspace, no atomics, no synchronisation.
 *
 *   p = cursor_dev ? *cursor_dev : position, as uint32;  epoch = p / num_batches,  pos = p % num_batches
 *   row = shuffle ? perm(seed, epoch, pos, num_batches) : pos
 *
 * For slot b with utterance u = batches[row][b]:  n = min(wave_len[u], n_out),  l = min(label_len[u], l_out);
 *   wave_out[b, :n]   = the utterance's samples,  wave_out[b, n:] = 0          wave_out: (batch, n_out) int16
 *   lengths_out[b]    = n                                                      (batch) int32
 *   labels_out[b, :l] = the utterance's labels,  the rest 0                    (batch, l_out) int32
 *   label_length_out[b] = l                                                    (batch) int32
 *   aux_out[b, :l]    = the utterance's aux words,  the rest -1                (batch, l_out) int32, or NULL
 *   utt_out[b]        = u                                                      (batch) int32, or NULL
 * An empty slot gives length 0, label length 0, all padding and utt_out = -1.
 *   plan = {p, epoch, pos, row}                                                QK_CORPUS_PLAN_WORDS int32, or NULL
 *
 * Every output element is written exactly once, whatever the buffers held before.  Nothing is read outside the rows the indices
 * name: a bad index is an empty slot, never an address; waveform reads are whole 16-byte groups of the utterance's own span (hence
 * the rounding of the layout above).  A cursor advanced by a device op between replays makes a captured graph gather a new batch
 * on every replay; cursor_dev is 4-byte aligned and wraps mod 2^32.
 *
 * perm(seed, epoch, pos, nb), uint32 arithmetic, fmix exactly as in the SpecAugment section of qk.h:
 *   k = the smallest even integer >= 2 with 2^k >= nb;  half = k / 2;  mask = 2^half - 1
 *   key = fmix(seed + 0x9E3779B1 * epoch)
 *   one pass:  L = x >> half, R = x & mask;  four rounds r = 0..3 of
 *              (L, R) <- (R, L ^ (fmix(key ^ (R * 0x9E3779B1 + r * 0x7F4A7C15 + 0x165667B1)) & mask));  x = (L << half) | R
 *   start from x = pos and repeat passes until x < nb.
 * A keyed Feistel bijection on [0, 2^k) restricted by cycle walking: a bijection on [0, nb) that always terminates.  The kernel
 * bounds the walk at 2^k passes (a bound no input reaches).
 *
 * Alignment: wave_pack 16 bytes; wave_out 2 bytes (any n_out, any row start: the body of every row is written with aligned 16-byte
 * stores, its head and tail element by element); every int32 / int64 array its natural alignment.  Outputs must not overlap inputs.
 *
 * QK_ERR_INVALID_ARG: a NULL corpus / schedule or a NULL required array (wave_pack, wave_off, wave_len, label_pack, label_off,
 *   label_len, batches, wave_out, lengths_out, labels_out, label_length_out); aux_out given without aux_pack; batch, num_batches,
 *   n_out or l_out below 1; num_utts, wave_samples or label_words below 0; shuffle not 0 or 1; a misaligned array.
 * QK_ERR_UNSUPPORTED: an output of 2^31 elements or more (batch * n_out or batch * l_out). */
int qk_corpus_batch(const qk_corpus_t *corpus, const qk_batch_schedule_t *schedule, uint32_t position, const uint32_t *cursor_dev,
                    int32_t n_out, int32_t l_out, int16_t *wave_out, int32_t *lengths_out, int32_t *labels_out,
                    int32_t *label_length_out, int32_t *aux_out, int32_t *utt_out, int32_t *plan, void *stream);

/* HOST only: out_host[pos] = perm(seed, epoch, pos, num_batches) for pos = 0 .. num_batches - 1, by the function the kernel
 * evaluates.  QK_ERR_INVALID_ARG: num_batches < 1 or a NULL out_host. */
int qk_epoch_permutation(uint32_t seed, uint32_t epoch, int32_t num_batches, int32_t *out_host);

#ifdef __cplusplus
}
#endif
#endif /* QK_DATA_H_ */
