// encoder_internal.h -- what csrc/rerank.hip sees of an encoder handle: the part of the forward that starts from tokens already
// on the device.  It stays inside the library (include/hiprag.h has no entry for it): the token ids index the embedding table
// unchecked, so only code that has range-checked them may write them.
#pragma once
#include "common.h"

namespace hiprag {

struct EncoderView {
    int device = 0, vocab = 0, pad_id = 0, max_pos = 0;
    bool has_head = false;
};

// A packed batch (encoder_packed.h) on the device: tokens [Tp] with pad in every sequence's granule tail, and packed_layout's
// tables.  real and sum_r2 are the layout's, for the FLOP count.
struct PackedBatch {
    const int32_t *tok, *lens, *row_off, *gran_seq, *items;
    int nseq, Tp, n_items;
    int64_t real;
    double sum_r2;
};

// Holds the encoder's mutex from acquire() until it is destroyed, and makes the encoder's device current.
class EncoderLease {
public:
    int32_t acquire(uint64_t h);   // HIPRAG_E_HANDLE for an unknown handle
    const EncoderView& view() const { return view_; }
    // the encoder's own token and length buffers, grown to `pairs` rows of S tokens
    int32_t reserve_tokens(size_t pairs, int S, int32_t** tok_dev, int32_t** lens_dev);
    // classification-head logits of nseq rows of S tokens (S a multiple of 64) that lie on the device, ordered on `st`
    int32_t score_dev(const int32_t* tok_dev, const int32_t* lens_dev, int nseq, int S, float* out_logits_dev, hipStream_t st);
    // the same for a packed batch: the encoder's token buffer grown to `rows` ints and its table buffer to `table_words` ints ...
    int32_t reserve_packed(size_t rows, size_t table_words, int32_t** tok_dev, int32_t** tab_dev);
    // ... its activation workspace grown to what a packed batch of Tp rows takes (before the first of several sub-batches
    // runs, so that no buffer grows under a forward that is still enqueued) ...
    int32_t reserve_packed_work(int Tp);
    // ... and the logits of a packed batch (Tp > 0, no sequence empty) that lies on the device, ordered on `st`
    int32_t score_packed_dev(const PackedBatch& b, float* out_logits_dev, hipStream_t st);

private:
    std::shared_ptr<void> enc_;
    std::unique_lock<std::mutex> lock_;
    EncoderView view_;
};

}  // namespace hiprag
