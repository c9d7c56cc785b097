// Internal view of the recompute encoder shared by encoder.hip (kernels, C ABI), api_index.hip
// (isl_set_recompute_provider) and search_recompute.hip (the rounds that re-encode the nodes a search misses).
#pragma once

#include "common.hpp"

struct isl_encoder {
  isl_bert_config cfg{};
  int device = -1;
  isl::DeviceBuffer<float> word, pos, type, eln_w, eln_b;
  struct Layer {
    isl::DeviceBuffer<float> wqkv, bqkv, wo, bo, ln1w, ln1b, wi, bi, wo2, bo2, ln2w, ln2b;
  };
  std::vector<Layer> layers;
  // optional reduced-precision mode: bf16 copies of the Linear weights (same order as `layers`)
  struct Layer16 { isl::DeviceBuffer<uint16_t> wqkv, wo, wi, wo2; };
  std::vector<Layer16> layers16;
  int32_t precision = 0;  // ISL_DTYPE_F32 / ISL_DTYPE_BF16
  // the buffers one model pass works in, grown on demand (tokens = sequences * padded length)
  struct Workspace {
    uint64_t tokens = 0;
    isl::DeviceBuffer<float> x, x1, t, qkv, ctx, inter;
    isl::DeviceBuffer<uint16_t> x16, x1_16;  // bf16 copies of x / x1 (bf16 mode)
    isl::DeviceBuffer<float> d_mask;
    isl::DeviceBuffer<int64_t> d_ids, d_tt;
  } ws;
  isl::DeviceBuffer<uint32_t> d_flag;  // an id out of range was met in a pass over ws
  // second workspace + stream (round 4): encoder_embed_nodes runs the two halves of a batch side by side,
  // so that one half's last, partly filled wave of GEMM tiles and its LayerNorm / attention kernels lie
  // beside the other half's GEMMs (a sequence's embedding does not depend on what it is batched with)
  struct Side {
    Workspace ws;
    isl::DeviceBuffer<uint32_t> d_flag;
    void* stream = nullptr;   // hipStream_t (non-blocking)
    void* ev_in = nullptr;    // hipEvent_t: the caller's stream up to the call
    void* ev_out = nullptr;   // hipEvent_t: the side stream's half is done
  } side;
  std::mutex mu;
};


namespace isl {
// Encodes the nodes listed in d_node_ids (device) from the resident token table (u16 ids, row i
// = node i, `L` slots per node, d_lens[i] of them used; NULL = all) and writes embedding b to
// d_rows + d_node_ids[b] * stride.  Sequences are padded to L: masked keys contribute exact
// zeros, so the result does not depend on the padded length.
// d_out_rows (device, may be NULL = the node ids): embedding b goes to d_rows + d_out_rows[b] * stride.
// batch sizes at which the passes of encoder_embed_nodes run whole waves of GEMM tiles (0 = unknown)
void encoder_batch_quantum(const isl_encoder* e, uint32_t L, uint32_t* quantum, uint32_t* chunk);
isl_status encoder_embed_nodes(isl_encoder* e, const uint16_t* d_tokens, const uint16_t* d_lens,
                               uint32_t L, const uint32_t* d_node_ids, uint64_t n, int normalize,
                               float* d_rows, uint64_t stride, hipStream_t st,
                               const uint32_t* d_out_rows = nullptr);
}  // namespace isl
