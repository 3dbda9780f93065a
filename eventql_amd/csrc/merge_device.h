// merge_device.h -- the device state behind an evql_merge_t made by evql_merge_create_device
// (merge.cc dispatches to it).
#pragma once
#include <vector>
#include "runtime.h"

namespace evql {

struct MergeDevice;

// EVQL_ENOTSUP: a select expression the device merge does not fold (count_distinct)
Status merge_device_create(evql_ctx* ctx, const std::vector<LoweredProgram>& select, MergeDevice** out);
void merge_device_destroy(MergeDevice* d);
int merge_device_ordinal(const MergeDevice* d);  // the context's device
Status merge_device_add_frame(MergeDevice* d, const void* payload, size_t len);
Status merge_device_add_rows(MergeDevice* d, const void* keys, size_t keys_len, const void* data,
                             size_t data_len, size_t nrows);
Status merge_device_num_groups(MergeDevice* d, uint64_t* out);
Status merge_device_next_batch(MergeDevice* d, size_t max_rows, evql_column_buf_t* cols, size_t* nrows);
void merge_device_stats(const MergeDevice* d, evql_merge_stats_t* out);

}  // namespace evql
