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

// Holds the encoder's mutex from acquire() until it is destroyed, and makes the encoder's device current.
class EncoderLease {
public:
    int32_t acquire(uint64_t h);   // HIPRAG_E_HANDLE for an unknown handle
    const EncoderView& view() const { return view_; }
    // the encoder's own token and length buffers, grown to `pairs` rows of S tokens
    int32_t reserve_tokens(size_t pairs, int S, int32_t** tok_dev, int32_t** lens_dev);
    // classification-head logits of nseq rows of S tokens (S a multiple of 64) that lie on the device, ordered on `st`
    int32_t score_dev(const int32_t* tok_dev, const int32_t* lens_dev, int nseq, int S, float* out_logits_dev, hipStream_t st);

private:
    std::shared_ptr<void> enc_;
    std::unique_lock<std::mutex> lock_;
    EncoderView view_;
};

}  // namespace hiprag
