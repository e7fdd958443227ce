// encoder_packed.h -- the layout of a PACKED encoder batch: sequences one after another, each rounded up to whole 64-row
// granules instead of to the batch's longest.  Host-only plain C++17 (no HIP header, no HIP type), like encoder_plan.h: pure
// arithmetic, so that Encoder::forward_packed (encoder.hip), the packed device rerank (rerank.hip) and a test on a machine
// without a GPU (hipenc_packed_layout) ask the same code.
//
//   sequence i of length len_i takes R_i = round_up(len_i, 64) rows (none if len_i == 0), starting at row_off[i], the prefix
//   sum of the R_i; Tp = row_off[nseq].  Rows [len_i, R_i) are padding: their token is pad_id, the embedding kernel writes
//   zeros there and attention masks those keys, exactly as in the padded layout.  Activations are [Tp][H]; q, k are
//   [heads][Tp][64] and V^T is [heads][64][Tp] -- what the QKV epilogues write when they are told of ONE sequence of Tp rows.
//   The granule is kSkinnyRows: the small-batch GEMM's row block and the attention's key tile, and it keeps every sequence's
//   V^T rows 16-byte aligned.
//
// The GEMM family depends on the row count alone: plan_forward(shape, 1, Tp) is the plan of a packed batch.
// The lexical and ColBERT heads have no packed form: hipenc_forward_lexical and hipenc_forward_colbert take padded batches only.
#pragma once
#include <cstdint>
#include <vector>

#include "encoder_plan.h"

namespace hiprag {

constexpr int kPackGranule = kSkinnyRows;   // 64
constexpr int kAttQueryTile = 128;          // attention2_kernel: queries per workgroup
constexpr int64_t kPackMaxRows = 1 << 30;   // Tp stays below this (hipenc_forward_plan's bound on nseq * S)

struct PackedLayout {
    std::vector<int32_t> row_off;    // [nseq + 1]
    std::vector<int32_t> gran_seq;   // [Tp / 64]: the sequence that owns each granule
    std::vector<int32_t> items;      // [n_items][2]: (seq, query tile j) for every 128 j < len_seq, in sequence order
    int32_t Tp = 0;
    int64_t real = 0;                // sum of the lengths
    double sum_r2 = 0.0;             // sum of R_i^2 (the attention term of the FLOP count)
    int n_items() const { return (int)(items.size() / 2); }
};

// false (and `out` unspecified) if a length is negative or Tp would reach kPackMaxRows
inline bool packed_layout(const int32_t* lens, int nseq, PackedLayout& out)
{
    out = PackedLayout{};
    out.row_off.assign((size_t)nseq + 1, 0);
    int64_t rows = 0;
    for (int i = 0; i < nseq; ++i) {
        if (lens[i] < 0) return false;
        out.row_off[i] = (int32_t)rows;
        const int64_t R = ((int64_t)lens[i] + kPackGranule - 1) / kPackGranule * kPackGranule;
        rows += R;
        if (rows >= kPackMaxRows) return false;
        out.real += lens[i];
        out.sum_r2 += (double)R * (double)R;
    }
    out.row_off[nseq] = out.Tp = (int32_t)rows;
    out.gran_seq.reserve((size_t)(rows / kPackGranule));
    for (int i = 0; i < nseq; ++i) {
        for (int g = out.row_off[i]; g < out.row_off[i + 1]; g += kPackGranule) out.gran_seq.push_back(i);
        for (int j = 0; j * kAttQueryTile < lens[i]; ++j) { out.items.push_back(i); out.items.push_back(j); }
    }
    return true;
}

}  // namespace hiprag
