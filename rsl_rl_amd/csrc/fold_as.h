// Internal interface of the partial-sum fold (mlp_wgrad.hip) for the units that fold with another problem's order.
#pragma once

#include "common.h"

namespace rslrl {

// rslrl_fold_partials_ex of NK columns in the summation order a fold of order_NK >= NK columns takes (which kernel runs
// and how the slices are grouped depend on the column count; an element's sum depends on that order alone): the bits
// of that wider fold's columns.  And its workspace.
int fold_partials_as(const float* partials, int64_t S, int64_t NK, int64_t order_NK, float* out, int64_t out_len,
                     int32_t t_rows, int32_t t_cols, void* workspace, size_t workspace_bytes, rslrl_stream_t stream);
size_t fold_partials_as_workspace_bytes(int64_t S, int64_t NK, int64_t order_NK);

}  // namespace rslrl
