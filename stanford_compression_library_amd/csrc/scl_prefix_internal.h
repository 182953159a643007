// scl_prefix_internal.h -- what the two prefix-code sources share: the device view of a code table and the model handle.
// scl_prefix.hip builds the tables (scl_prefix_model_create) and holds the batched kernels, one lane per chunk;
// scl_prefix_block.hip codes one large block with the whole grid from the same tables.
#pragma once

#include "scl_common.h"

#define PF_MAX_LEN 32u
#define PF_LUT_BITS 11u  // 2^11 16-bit entries = 4 KiB: with the 32 KiB ring and the deep nodes four workgroups per CU
#define PF_DEEP_NODES 512u

// a child in the any-parameter tree (uint2 {child on 0, child on 1} per node, node 0 = root)
#define PF_NONE 0xFFFFFFFFu
#define PF_LEAF 0x80000000u  // | symbol
// a child in the tuned decoder's deep-node table (two u16 per node: low half = child on 0)
#define PF16_NONE 0xFFFFu
#define PF16_LEAF 0x8000u  // | symbol
// a lookup-table entry: len in bits 0..3, kind in bits 4..5, symbol / deep node in bits 6..15
#define PF_KIND_SYM 0u
#define PF_KIND_NODE 1u  // len = T: the walk continues at deep node `payload`
#define PF_KIND_NONE 2u  // len = number of bits read when the walk meets a missing child

struct PrefixDev {
    u32 K;
    u32 min_len, max_len;
    u32 lut_bits;  // T
    u32 n_deep;
    u32 len_gcd;           // gcd of all code lengths: every codeword boundary of a stream is a multiple of it
    const uint2 *d_enc;    // [max(K, 256)] {code, len}
    const uint2 *d_nodes;  // any-parameter decoder
    const u16 *d_lut;      // tuned decoder: [2^T]
    const u32 *d_deep;     // tuned decoder: [n_deep]
};

struct scl_prefix_model {
    int device;
    PrefixDev dev;
    u32 fast;
    uint2 *d_enc, *d_nodes;
    u16 *d_lut;
    u32 *d_deep;
};
