// scl_lz77_entropy.hip -- the entropy stage of LZ77 for gfx950: sequences and literals <-> the reference's block bits, for
// a batch of streams.
//
//   scl_lz77_entropy_encode_batch  <->  LZ77StreamsEncoder.encode_block   scl/compressors/lz77.py:301-361
//   scl_lz77_entropy_decode_batch  <->  LZ77StreamsDecoder.decode_block   scl/compressors/lz77.py:364-428
//
// ONE WAVEFRONT (one workgroup of 64 threads) PER STREAM.  A stream is four fields in a fixed order -- literal counts,
// match lengths, match offsets (log-scale binned, :212-298), literals -- and each field is
//   [32-bit counts_size][Elias-delta code of every count of the alphabet][32-bit values_size][Huffman codewords][residuals]
// (:127-209) under the Huffman code of the field's own counts (scl_lz77_huffman.h).  A field with no values is one zero
// header.  The encoder knows every size before it stores a bit (histograms -> trees -> sizes), so a stream that does not
// fit stores nothing; the decoder walks field after field and stops at its first fault.  No workgroup waits on another,
// every loop is bounded by the data, and nothing outside a stream's own slot / input bits / rows / literal range is touched.
// The step from histograms to code tables (lze_build_codes) and the counts parser (lze_parse_counts) are the ones the wide
// stage uses: scl_lz77_entropy_internal.h.
#include "scl_lz77_entropy_internal.h"

namespace {

#define LZE_THREADS SCL_WAVE
#define LZE_STAGE_WORDS 96u  // 64 codewords of at most 43 bits behind at most 31 pending bits: 87 words
#define LZE_MAX_GRID (1u << 20)

__device__ __forceinline__ u64 lze_wave_sum(u64 v) {
#pragma unroll
    for (u32 d = 32; d; d >>= 1) {
        const u32 lo = __shfl_xor((u32)v, d), hi = __shfl_xor((u32)(v >> 32), d);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// ---- the wave's bit appender -----------------------------------------------------------------------------------------
// append(): lane i hands in the low `len` bits of `val` (MSB first, len <= 43); the 64 codewords go behind the stream in
// lane order.  They are assembled in LDS with atomic ORs; whole 32-bit big-endian words leave for the slot, the last partial
// word stays in stage[0] for the next call.  Words that would not lie inside the slot are not stored.
struct LzeWriter {
    u32 *stage;
    u8 *slot;
    u64 slot_bytes, pos;

    __device__ __forceinline__ void init(u32 *stage_, u8 *slot_, u64 slot_bytes_) {
        stage = stage_;
        slot = slot_;
        slot_bytes = slot_bytes_;
        pos = 0;
        for (u32 w = lz_lane(); w < LZE_STAGE_WORDS; w += SCL_WAVE) stage[w] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void store_word(u64 w, u32 v) {
        if ((w + 1) * 4 <= slot_bytes) reinterpret_cast<u32 *>(slot)[w] = scl_bswap32(v);
    }
    __device__ __forceinline__ void append(u64 val, u32 len) {
        u32 total;
        const u32 off = scl_wave_scan_excl<u32, SclScanSum>(len, &total);
        if (total == 0) return;  // wave-uniform
        const u32 pend = (u32)(pos & 31);
        if (len) {
            const u32 b = pend + off, w = b >> 5, sh = b & 31;
            const u64 top = val << (64 - len);
            const u64 t = top >> sh;
            const u32 w0 = (u32)(t >> 32), w1 = (u32)t, w2 = sh ? (u32)((top << (64 - sh)) >> 32) : 0u;
            if (w0) atomicOr(&stage[w], w0);
            if (w1 && w + 1 < LZE_STAGE_WORDS) atomicOr(&stage[w + 1], w1);
            if (w2 && w + 2 < LZE_STAGE_WORDS) atomicOr(&stage[w + 2], w2);
        }
        __syncthreads();
        const u32 n_full = (pend + total) >> 5;
        const u64 first = pos >> 5;
        for (u32 w = lz_lane(); w < n_full; w += SCL_WAVE) store_word(first + w, stage[w]);
        const u32 carry = stage[n_full];
        __syncthreads();
        for (u32 w = lz_lane(); w <= n_full; w += SCL_WAVE) stage[w] = w == 0 ? carry : 0u;
        __syncthreads();
        pos += total;
    }
    __device__ __forceinline__ void header(u32 v) {
        const bool first = lz_lane() == 0;
        append(first ? v : 0u, first ? 32u : 0u);
    }
    __device__ __forceinline__ void finish() {  // the last partial word, zero bits behind the stream
        if ((pos & 31) && lz_lane() == 0) store_word(pos >> 5, stage[0]);
    }
};

// ---- encode ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LZE_THREADS) void lz77_entropy_encode(
    u64 n_streams, u32 seq_cap, u32 o, const u32 *lit_count, const u32 *match_len, const u32 *match_off, const u32 *n_seq_in,
    const u8 *literals, u64 lit_bytes, const u64 *lit_off, const u32 *n_lit_in, u8 *out, u64 out_stride, u64 *bit_off_out,
    u32 *nbits_out, u32 *status_out) {
    __shared__ u32 hist[LZE_SYMS], code[LZE_SYMS];
    __shared__ u8 clen[LZE_SYMS];
    __shared__ LzeSmallTree small[3];
    __shared__ LzeBigTree big;
    __shared__ u32 stage[LZE_STAGE_WORDS];
    __shared__ u32 n_leaves[4], counts_size[4], values_size[4], flags;
    const u32 lane = lz_lane();
    const u32 A = 32 + o;  // a sequence field's alphabet

    for (u64 s = blockIdx.x; s < n_streams; s += gridDim.x) {
        const u32 n_seq = n_seq_in[s], n_lit = n_lit_in[s];
        const u64 l_at = lit_off[s];
        u32 status = 0;
        u64 total_bits = 0;
        if (n_seq > seq_cap || l_at > lit_bytes || n_lit > lit_bytes - l_at) {
            status = SCL_ST_SIZE;
        } else {
            const u32 *row0 = lit_count + s * seq_cap, *row1 = match_len + s * seq_cap, *row2 = match_off + s * seq_cap;
            const u8 *lit = literals + l_at;
            // histograms
            for (u32 j = lane; j < LZE_SYMS; j += SCL_WAVE) hist[j] = 0;
            if (lane == 0) flags = 0;
            __syncthreads();
            for (u32 f = 0; f < 3; ++f) {
                const u32 *row = f == 0 ? row0 : f == 1 ? row1 : row2;
                for (u64 k = lane; k < n_seq; k += SCL_WAVE) {
                    u32 log, res;
                    const u32 b = lze_bin(row[k], o, &log, &res);
                    if (b < A)
                        atomicAdd(&hist[f * LZE_FIELD_K + b], 1u);
                    else
                        atomicOr(&flags, SCL_ST_SYMBOL);
                }
            }
            for (u64 k = lane; k < n_lit; k += SCL_WAVE) atomicAdd(&hist[LZE_LIT_BASE + lit[k]], 1u);
            __syncthreads();
            // the four trees, one lane each, and the code tables
            lze_build_codes<LZE_THREADS>(hist, A, lane, small, big, n_leaves, code, clen, &flags);
            status = flags;
            // sizes
            for (u32 f = 0; f < 4; ++f) {
                const u32 base = f * LZE_FIELD_K, K = f < 3 ? A : 256u, n = f < 3 ? n_seq : n_lit;
                u64 cs = 0, vs = 0, rs = 0;
                if (n && status == 0) {
                    for (u32 j = lane; j < K; j += SCL_WAVE) {
                        const u32 c = hist[base + j];
                        u64 val;
                        cs += lze_elias_delta(c, &val);
                        if (c) vs += (u64)c * clen[base + j];
                        if (f < 3 && j >= o) rs += (u64)c * (j - o);
                    }
                    cs = lze_wave_sum(cs);
                    vs = lze_wave_sum(vs);
                    rs = lze_wave_sum(rs);
                }
                if (lane == 0) {
                    counts_size[f] = (u32)cs;
                    values_size[f] = (u32)vs;
                }
                if (vs >> 32) total_bits = 1ull << 32;  // does not fit its own header
                total_bits += n ? 64 + cs + vs + rs : 32;
            }
            if (status) {
                total_bits = 0;
            } else if (total_bits >> 32) {
                status = SCL_ST_CAPACITY;
                total_bits = 0xFFFFFFFFull;
            } else if ((total_bits + 7) / 8 > out_stride) {
                status = SCL_ST_CAPACITY;
            } else {
                LzeWriter wr;
                wr.init(stage, out + s * out_stride, out_stride);  // (its barrier publishes the sizes)
                for (u32 f = 0; f < 4; ++f) {
                    const u32 base = f * LZE_FIELD_K, K = f < 3 ? A : 256u, n = f < 3 ? n_seq : n_lit;
                    const u32 *row = f == 0 ? row0 : f == 1 ? row1 : row2;  // (unused for the literals)
                    if (n == 0) {
                        wr.header(0);
                        continue;
                    }
                    wr.header(counts_size[f]);
                    for (u32 j0 = 0; j0 < K; j0 += SCL_WAVE) {
                        u64 val = 0;
                        u32 len = 0;
                        if (j0 + lane < K) len = lze_elias_delta(hist[base + j0 + lane], &val);
                        wr.append(val, len);
                    }
                    wr.header(values_size[f]);
                    for (u64 k0 = 0; k0 < n; k0 += SCL_WAVE) {
                        u32 val = 0, len = 0;
                        if (k0 + lane < n) {
                            u32 log, res;
                            const u32 sym = f < 3 ? lze_bin(row[k0 + lane], o, &log, &res) : lit[k0 + lane];
                            val = code[base + sym];
                            len = clen[base + sym];
                        }
                        wr.append(val, len);
                    }
                    if (f < 3)
                        for (u64 k0 = 0; k0 < n; k0 += SCL_WAVE) {
                            u32 log = 0, res = 0;
                            if (k0 + lane < n) lze_bin(row[k0 + lane], o, &log, &res);
                            wr.append(res, log);
                        }
                }
                wr.finish();
            }
        }
        if (lane == 0) {
            bit_off_out[s] = 8 * s * out_stride;
            nbits_out[s] = (u32)total_bits;
            status_out[s] = status;
        }
        __syncthreads();  // the next stream reuses the tables
    }
}

// ---- decode ----------------------------------------------------------------------------------------------------------
// (lze_read_bits and the one-lane cursor LzeCursor: scl_lz77_entropy_internal.h)
__global__ __launch_bounds__(LZE_THREADS) void lz77_entropy_decode(
    const u8 *in, u64 in_size_bytes, const u64 *bit_off, const u32 *in_nbits, u64 n_streams, u32 seq_cap, u32 o,
    u32 *lit_count, u32 *match_len, u32 *match_off, u32 *n_seq_out, u8 *literals, u64 lit_bytes, const u64 *lit_off,
    const u32 *lit_cap_in, u32 *n_lit_out, u32 *consumed_out, u32 *status_out) {
    __shared__ u32 hist[LZ_HUFF_MAX_K];
    __shared__ LzeBigTree tree;
    __shared__ u32 sh_m, sh_count, sh_status, sh_resid;
    const u32 lane = lz_lane();

    for (u64 s = blockIdx.x; s < n_streams; s += gridDim.x) {
        const u64 at = bit_off[s], nbits = in_nbits[s], l_at = lit_off[s];
        const u32 lit_cap = lit_cap_in[s];
        u32 status = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;  // values decoded per field
        u64 pos = 0;  // bits of the stream used so far
        if (at > in_size_bytes * 8 || nbits > in_size_bytes * 8 - at || l_at > lit_bytes || lit_cap > lit_bytes - l_at) {
            status = SCL_ST_SIZE;
        } else {
            u32 *row0 = lit_count + s * seq_cap, *row1 = match_len + s * seq_cap, *row2 = match_off + s * seq_cap;
            u8 *lit = literals + l_at;
            for (u32 f = 0; f < 4 && status == 0; ++f) {
                const u32 K = f < 3 ? 32 + o : 256u, cap = f < 3 ? seq_cap : lit_cap;
                u32 *row_f = f == 0 ? row0 : f == 1 ? row1 : row2;  // (unused for the literals)
                if (pos + 32 > nbits) {
                    status = SCL_ST_TRUNCATED;
                    break;
                }
                const u32 counts_size = lze_read_bits(in, at + pos, 32);
                pos += 32;
                if (counts_size == 0) continue;
                if (pos + counts_size > nbits) {
                    status = SCL_ST_TRUNCATED;
                    break;
                }
                for (u32 j = lane; j < LZ_HUFF_MAX_K; j += SCL_WAVE) hist[j] = 0;
                if (lane == 0) sh_status = sh_resid = 0;
                __syncthreads();
                if (lane == 0) sh_status = lze_parse_counts(in, at + pos, counts_size, K, hist);
                __syncthreads();
                status = sh_status;
                if (status) break;
                pos += counts_size;
                if (pos + 32 > nbits) {
                    status = SCL_ST_TRUNCATED;
                    break;
                }
                const u32 values_size = lze_read_bits(in, at + pos, 32);
                pos += 32;
                if (pos + values_size > nbits) {
                    status = SCL_ST_TRUNCATED;
                    break;
                }
                if (lane == 0) {
                    const LzHuffTree t = {tree.prob, tree.heap, tree.parent, tree.kids, tree.leaf_sym};
                    sh_m = lz_huffman_build(hist, K, t);
                }
                __syncthreads();
                const u32 m = sh_m;
                for (u32 i = lane; i < m; i += SCL_WAVE) {
                    u32 c;
                    if (lz_huffman_leaf_code(tree.parent, i, &c) > LZ_HUFF_MAX_CODE_BITS) atomicOr(&sh_status, SCL_ST_SIZE);
                }
                __syncthreads();
                status = sh_status;
                __syncthreads();  // every lane has read it before lane 0 writes the walk's
                if (status) break;
                if (lane == 0) {  // walk the tree down values_size bits
                    LzeCursor cur;
                    cur.init(in, at + pos, values_size);
                    const u32 root = lz_huffman_root(m);
                    u32 node = root, n_out = 0, st = 0;
                    while (cur.left) {
                        const u32 child = tree.kids[2 * (node - m) + cur.get(1)];
                        if (child == LZ_HUFF_NONE) {
                            st = SCL_ST_STATE;
                            break;
                        }
                        if (child >= m) {
                            node = child;
                            continue;
                        }
                        if (n_out >= cap) {
                            st = SCL_ST_CAPACITY;
                            break;
                        }
                        if (f < 3)
                            row_f[n_out] = tree.leaf_sym[child];
                        else
                            lit[n_out] = (u8)tree.leaf_sym[child];
                        ++n_out;
                        node = root;
                    }
                    if (st == 0 && node != root) st = SCL_ST_STATE;  // a cut codeword
                    sh_count = n_out;
                    sh_status = st;
                }
                // the bins lane 0 stored are read back by every lane
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __syncthreads();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const u32 n = sh_count;
                if (f == 0) c0 = n;
                if (f == 1) c1 = n;
                if (f == 2) c2 = n;
                if (f == 3) c3 = n;
                status = sh_status;
                if (status) break;
                pos += values_size;
                if (f < 3) {  // the residuals, 64 values at a time (a fault here leaves bins behind the values already made)
                    volatile u32 *row = row_f;
                    for (u64 k0 = 0; k0 < n; k0 += SCL_WAVE) {
                        const bool live = k0 + lane < n;
                        const u32 b = live ? row[k0 + lane] : 0u;
                        const u32 log = b >= o ? b - o : 0u;
                        u32 total;
                        const u32 off = scl_wave_scan_excl<u32, SclScanSum>(log, &total);
                        if (pos + total > nbits) {
                            status = SCL_ST_TRUNCATED;
                            break;
                        }
                        if (live && b >= o) {
                            const u64 v = (u64)o + (1ull << log) + lze_read_bits(in, at + pos + off, log) - 1;
                            if (v >> 32)
                                atomicOr(&sh_resid, SCL_ST_STATE);  // no 32-bit field holds it
                            else
                                row[k0 + lane] = (u32)v;
                        }
                        pos += total;
                    }
                    __syncthreads();
                    status |= sh_resid;
                    __syncthreads();  // read by every lane before the next field clears it
                }
            }
        }
        const u32 n_seq = min(c0, min(c1, c2));
        if (status == 0 && (c0 != n_seq || c1 != n_seq || c2 != n_seq)) status = SCL_ST_STATE;
        if (lane == 0) {
            n_seq_out[s] = n_seq;
            n_lit_out[s] = c3;
            consumed_out[s] = (u32)pos;
            status_out[s] = status;
        }
        __syncthreads();
    }
}

u32 lze_grid(u64 n_streams) { return (u32)(n_streams < LZE_MAX_GRID ? n_streams : LZE_MAX_GRID); }

}  // namespace

extern "C" uint64_t scl_lz77_entropy_slot_bytes(uint64_t max_n_seq, uint64_t max_n_lit, uint32_t binned_offset) {
    // per field two headers and the counts (at most 43 bits each), and 31 residual bits per sequence value.  The codewords
    // of a field of n values take less than n * (H + 1) bits IN TOTAL under the Huffman code of the field's own counts, H
    // their empirical entropy <= log2 K: n * 7 with K = 64 (holds every sequence alphabet), n * 9 for the literals.  A bound
    // on the field, not on a codeword: a single codeword may have 32 bits.
    const u64 o = binned_offset <= 32 ? binned_offset : 32;
    const u64 bits = 3 * (64 + 43 * (32 + o) + max_n_seq * (7 + 31)) + 64 + 43 * 256 + max_n_lit * 9;
    return scl_round_up(bits / 8 + 8, 128);
}

extern "C" int scl_lz77_entropy_kernel_names(char *enc, char *dec, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_entropy_kernel_names: cap must be at least 96");
    if (enc) snprintf(enc, cap, "lz77_entropy_encode");
    if (dec) snprintf(dec, cap, "lz77_entropy_decode");
    return SCL_OK;
}

extern "C" int scl_lz77_entropy_encode_batch(const scl_lz77_entropy_encode_args *a, void *stream) {
    const char *what = "lz77_entropy_encode_batch";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_n_seq && a->d_lit_off && a->d_n_lit && a->d_out && a->d_bit_off && a->d_nbits && a->d_status &&
                    (a->lit_bytes == 0 || a->d_literals) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->binned_offset <= 32, "%s: binned_offset %u: 0 <= binned_offset <= 32", what, a->binned_offset);
    SCL_REQUIRE(a->n_streams < (1ull << 32), "%s: a batch holds less than 2^32 streams", what);
    SCL_REQUIRE(a->out_stride % 16 == 0 && a->out_stride > 0 && ((uintptr_t)a->d_out & 15) == 0,
                "%s: out_stride must be a positive multiple of 16 and d_out 16-byte aligned", what);
    if (a->n_streams == 0) return SCL_OK;
    hipLaunchKernelGGL(lz77_entropy_encode, dim3(lze_grid(a->n_streams)), dim3(LZE_THREADS), 0, (hipStream_t)stream,
                       a->n_streams, a->seq_cap, a->binned_offset, a->d_lit_count, a->d_match_len, a->d_match_off,
                       a->d_n_seq, a->d_literals, a->lit_bytes, a->d_lit_off, a->d_n_lit, a->d_out, a->out_stride,
                       a->d_bit_off, a->d_nbits, a->d_status);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_lz77_entropy_decode_batch(const scl_lz77_entropy_decode_args *a, void *stream) {
    const char *what = "lz77_entropy_decode_batch";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_bit_off && a->d_in_nbits && a->d_n_seq && a->d_lit_off && a->d_lit_cap && a->d_n_lit &&
                    a->d_consumed && a->d_status && (a->in_size_bytes == 0 || a->d_in) &&
                    (a->lit_bytes == 0 || a->d_literals) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->binned_offset <= 32, "%s: binned_offset %u: 0 <= binned_offset <= 32", what, a->binned_offset);
    SCL_REQUIRE(a->n_streams < (1ull << 32), "%s: a batch holds less than 2^32 streams", what);
    SCL_REQUIRE(a->in_size_bytes < (1ull << 60), "%s: in_size_bytes must be below 2^60", what);
    if (a->n_streams == 0) return SCL_OK;
    hipLaunchKernelGGL(lz77_entropy_decode, dim3(lze_grid(a->n_streams)), dim3(LZE_THREADS), 0, (hipStream_t)stream,
                       a->d_in, a->in_size_bytes, a->d_bit_off, a->d_in_nbits, a->n_streams, a->seq_cap, a->binned_offset,
                       a->d_lit_count, a->d_match_len, a->d_match_off, a->d_n_seq, a->d_literals, a->lit_bytes,
                       a->d_lit_off, a->d_lit_cap, a->d_n_lit, a->d_consumed, a->d_status);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

// the shared tree builder on the host: code[i] / len[i] of every symbol with a count (0 / 0 for the others)
extern "C" int scl_lz77_huffman_from_counts_host(const uint64_t *counts, uint32_t K, uint32_t *code, uint8_t *len) {
    const char *what = "lz77_huffman_from_counts_host";
    SCL_REQUIRE(counts && code && len, "%s: null pointer argument", what);
    SCL_REQUIRE(K >= 1 && K <= LZ_HUFF_MAX_K, "%s: K = %u: 1 <= K <= 256", what, K);
    u64 total = 0;
    for (u32 i = 0; i < K; ++i) {
        SCL_REQUIRE(counts[i] < (1ull << 32), "%s: counts are below 2^32", what);
        total += counts[i];
    }
    SCL_REQUIRE(total > 0, "%s: every count is zero: there is no alphabet", what);
    double prob[2 * LZ_HUFF_MAX_K];
    u16 heap[LZ_HUFF_MAX_K], parent[2 * LZ_HUFF_MAX_K], leaf_sym[LZ_HUFF_MAX_K];
    const LzHuffTree t = {prob, heap, parent, nullptr, leaf_sym};
    const u32 m = lz_huffman_build(counts, K, t);
    for (u32 i = 0; i < K; ++i) {
        code[i] = 0;
        len[i] = 0;
    }
    for (u32 i = 0; i < m; ++i) {
        u32 c;
        const u32 l = lz_huffman_leaf_code(parent, i, &c);
        SCL_REQUIRE(l <= LZ_HUFF_MAX_CODE_BITS, "%s: symbol %u gets a codeword of %u bits: the kernels code up to 32", what,
                    (u32)leaf_sym[i], l);
        code[leaf_sym[i]] = c;
        len[leaf_sym[i]] = (u8)l;
    }
    return SCL_OK;
}
