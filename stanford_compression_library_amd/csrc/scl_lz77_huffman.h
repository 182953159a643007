// scl_lz77_huffman.h -- the Huffman tree of LZ77's entropy stage, by the reference's rule, as ONE function for host and
// device (scl_lz77_entropy.hip).  Internal to csrc/.
//
// The rule (scl/compressors/huffman_coder.py:38-93 over Python's heapq): one leaf per symbol with count > 0 in ascending
// symbol order, prob = double(count) / double(total); heapify; then pop first (left, bit 0), pop second (right, bit 1), push
// a node with the double sum.  "a < b" is a.prob <= b.prob and nothing else, so which of two equal nodes comes out first is
// decided by the sift order alone: _siftup / _siftdown / heappop / heappush below follow heapq's source step for step.
#pragma once

#include "scl_common.h"

#ifdef __HIPCC__
#define LZ_HD __host__ __device__
#else
#define LZ_HD
#endif

#define LZ_HUFF_MAX_K 256u
#define LZ_HUFF_NONE 0xFFFFu      // no parent (the root) / no child (the right child of the one-symbol code's root)
#define LZ_HUFF_RIGHT 0x8000u     // in parent[]: the node is its parent's right child (bit 1)
#define LZ_HUFF_MAX_CODE_BITS 32u

// Views into the caller's storage (LDS on the device, the stack on the host) for an alphabet of K symbols.  Nodes 0..m-1
// are the leaves (m = symbols with a count), m..2m-2 the inner nodes in the order they were made; the root is the last.
struct LzHuffTree {
    double *prob;   // [2K]
    u16 *heap;      // [K]
    u16 *parent;    // [2K]  parent | LZ_HUFF_RIGHT, the root: LZ_HUFF_NONE
    u16 *kids;      // [2K] or nullptr: kids[2 * (j - m)] / [2 * (j - m) + 1] = left / right child of inner node j
    u16 *leaf_sym;  // [K]   the symbol of leaf i
};

// heapq._siftdown(heap, startpos, pos)
LZ_HD inline void lz_heap_siftdown(const double *prob, u16 *heap, u32 startpos, u32 pos) {
    const u16 item = heap[pos];
    const double p = prob[item];
    while (pos > startpos) {
        const u32 parentpos = (pos - 1) >> 1;
        const u16 par = heap[parentpos];
        if (p <= prob[par]) {  // newitem < parent
            heap[pos] = par;
            pos = parentpos;
            continue;
        }
        break;
    }
    heap[pos] = item;
}

// heapq._siftup(heap, pos): down to a leaf along the smaller children, then back up
LZ_HD inline void lz_heap_siftup(const double *prob, u16 *heap, u32 n, u32 pos) {
    const u32 startpos = pos;
    const u16 item = heap[pos];
    u32 childpos = 2 * pos + 1;
    while (childpos < n) {
        const u32 rightpos = childpos + 1;
        if (rightpos < n && !(prob[heap[childpos]] <= prob[heap[rightpos]])) childpos = rightpos;
        heap[pos] = heap[childpos];
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    heap[pos] = item;
    lz_heap_siftdown(prob, heap, startpos, pos);
}

// heapq.heappop(heap): the last element goes to the root
LZ_HD inline u16 lz_heap_pop(const double *prob, u16 *heap, u32 *n) {
    const u16 last = heap[--*n];
    if (*n) {
        const u16 ret = heap[0];
        heap[0] = last;
        lz_heap_siftup(prob, heap, *n, 0);
        return ret;
    }
    return last;
}

// -> m, the number of symbols with a count (0: no tree).  The root is node lz_huffman_root(m).
template <class CNT>
LZ_HD inline u32 lz_huffman_build(const CNT *counts, u32 K, const LzHuffTree &t) {
    u64 total = 0;
    for (u32 i = 0; i < K; ++i) total += counts[i];
    u32 m = 0;
    for (u32 i = 0; i < K; ++i)
        if (counts[i]) {
            t.prob[m] = (double)counts[i] / (double)total;
            t.heap[m] = (u16)m;
            t.leaf_sym[m] = (u16)i;
            ++m;
        }
    if (m == 0) return 0;
    if (m == 1) {  // the code "0": a root with a left child only
        t.parent[0] = 1;
        t.parent[1] = LZ_HUFF_NONE;
        if (t.kids) {
            t.kids[0] = 0;
            t.kids[1] = LZ_HUFF_NONE;
        }
        return 1;
    }
    for (u32 i = m / 2; i-- > 0;) lz_heap_siftup(t.prob, t.heap, m, i);  // heapq.heapify
    u32 n = m, next = m;
    while (n > 1) {
        const u16 a = lz_heap_pop(t.prob, t.heap, &n);
        const u16 b = lz_heap_pop(t.prob, t.heap, &n);
        t.prob[next] = t.prob[a] + t.prob[b];
        t.parent[a] = (u16)next;
        t.parent[b] = (u16)(next | LZ_HUFF_RIGHT);
        if (t.kids) {
            t.kids[2 * (next - m)] = a;
            t.kids[2 * (next - m) + 1] = b;
        }
        t.heap[n] = (u16)next;  // heapq.heappush
        lz_heap_siftdown(t.prob, t.heap, 0, n);
        ++n;
        ++next;
    }
    t.parent[next - 1] = LZ_HUFF_NONE;
    return m;
}

LZ_HD inline u32 lz_huffman_root(u32 m) { return m == 1 ? 1u : 2 * m - 2; }

// the codeword of leaf `leaf`: -> its length; *code = its bits, most significant first in the low `length` bits (only the
// last 32 are kept: a length above LZ_HUFF_MAX_CODE_BITS is the caller's to refuse)
LZ_HD inline u32 lz_huffman_leaf_code(const u16 *parent, u32 leaf, u32 *code) {
    u32 c = 0, depth = 0, j = leaf;
    while (parent[j] != LZ_HUFF_NONE) {
        const u16 p = parent[j];
        if (depth < 32 && (p & LZ_HUFF_RIGHT)) c |= 1u << depth;
        ++depth;
        j = p & (LZ_HUFF_RIGHT - 1);
    }
    *code = c;
    return depth;
}
