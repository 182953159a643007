// scl_lz77_entropy_wide.hip -- the entropy stage of ONE large LZ77 stream across the whole GPU, for gfx950.
//
// scl_lz77_entropy.hip gives a stream one wavefront, and its decoder walks every codeword with one lane.  Here the same bits
// (the layout of include/scl_hip.h: four fields, each [32-bit counts_size][Elias-delta counts][32-bit values_size][Huffman
// codewords][residual bits]) are written and read by every CU.
//
// encode   lzw_hist        grid-wide histograms of the three binned fields and the literals: LDS per workgroup, merged with
//                          global atomics; a value without a bin raises SCL_ST_SYMBOL
//          lzw_layout      ONE workgroup: four lanes build the four trees (lz_huffman_build), the code tables go to scratch,
//                          every section size is a sum over the alphabet, so the 64-bit position of every header and section
//                          and every fault are known before a bit is stored
//          lzw_zero        the words of the stream are zeroed (the emitters OR into shared words); a faulted stream: nothing
//          lzw_heads       one workgroup per field: the two headers and the Elias-delta counts, ORed in at any bit position
//          lzw_tile_bits / lzw_scan_tiles / lzw_emit   as pfb_tile_bits / pfb_scan_tiles / pfb_encode_tile of
//                          scl_prefix_block.hip over the seven sections at once -- the codewords of four fields, the residuals
//                          of three: a codeword tile takes {code, len} of bin(v), a residual tile (residual(v), log(v)), from
//                          a section base at any bit.  lzw_tile_bits and lzw_emit are the ONE copy of those bodies
//                          (pfb_tile_bits_body, pfb_encode_tile_body, scl_bit_block.h) over the value policy LzwEnc; the
//                          last, partial word of out_cap_bytes % 4 != 0 is that header's pfb_encode_tail_kernel
// decode   field by field (a field starts where the one before it ended, and the residuals' length is known only from the
//          decoded bins); the host reads one small struct per field and two words per pass:
//          lzw_dec_head    ONE workgroup: the headers, the Elias-delta counts (one lane: at most 256 codewords), the tree, a
//                          2^9 lookup table and the node array in scratch; every fault of the one-lane decoder in its order
//          lzw_sync / lzw_scan_groups / lzw_write   the self-synchronising scheme of scl_prefix_block.hip (Weissenberger &
//                          Schmidt) from the ONE copy of its bodies (pfb_sync_body, pfb_scan_to_end, pfb_write_body and the
//                          host's pass loop pfb_decode_section, scl_bit_block.h).  Owned here: the codeword policy LzwCode over
//                          the device-built tree (a cut codeword and a missing child both end a walk as PFB_END_STATE), the
//                          section's bit base, and the LZ77 one-lane decoder's verdict in lzw_scan_groups (a cut is
//                          SCL_ST_STATE, SCL_ST_CAPACITY is decided at the leaf behind the cap)
//          lzw_resid_bits / lzw_resid_scan / lzw_resid   the bins become values: a 64-bit scan of the residual widths over
//                          tiles of 4096 gives each value its bits; the one-lane decoder's step of 64 values decides where a
//                          truncated section stops counting
//          lzw_finish      the result
// No kernel waits on another workgroup: no flag is spun on, no look-back, no cooperative launch.  Every loop is bounded by
// the data.  LDS per workgroup: layout 15 KiB, tile kernels 3.5 KiB of tables + 16.4 KiB of words, sync / write 3.5 KiB of
// tables + 4.3 KiB of input + 1 KiB of exits -- four workgroups per CU fit everywhere.
#include "scl_bit_block.h"
#include "scl_lz77_entropy_internal.h"

namespace {

#define LZW_HIST_MAX_GRID 1024u
#define LZW_ZERO_MAX_GRID 2048u
#define LZW_LUT_BITS 9u
#define LZW_LUT_SIZE (1u << LZW_LUT_BITS)
#define LZW_KIND_LEAF 0u  // entry = kind << 30 | length << 16 | symbol
#define LZW_KIND_NODE 1u  //                                   | inner node reached after LZW_LUT_BITS bits
#define LZW_KIND_NONE 2u  //                                     the missing child of the one-symbol code, at bit `length`
#define LZW_NONE32 0xFFFFFFFFu
#define LZW_SECTIONS 7u   // 2 f: the codewords of sequence field f, 2 f + 1: its residuals, 6: the literals' codewords

// ---- encode ---------------------------------------------------------------------------------------------------------------
struct LzwEncHead {      // head of the encoder's scratch (256 bytes, zeroed by the entry point)
    PfbEncScratch tile;  // fits, tail_word
    u32 flags, pad;      // lzw_hist: SCL_ST_SYMBOL
    u64 total_bits;
    u64 field_at[4];     // bit of the field's first header
    u64 section_at[8];   // bit of section s (LZW_SECTIONS of them)
    u32 counts_size[4], values_size[4];
};

struct LzwEncIn {
    const u32 *row[3];
    const u8 *lit;
    u32 n_seq, n_lit, o;
};

struct LzwEncScratch {
    LzwEncHead *head;
    u32 *hist;       // [LZE_SYMS]
    uint2 *enc;      // [LZE_SYMS] {code, len}
    u64 *tile_bits;  // [6 * tiles(n_seq) + tiles(n_lit)]
};

__device__ __forceinline__ const u32 *lzw_row(const LzwEncIn &in, u32 f) { return f == 0 ? in.row[0] : f == 1 ? in.row[1] : in.row[2]; }

__global__ void __launch_bounds__(PFB_THREADS) lzw_hist_kernel(LzwEncIn in, LzwEncScratch sc) {
    __shared__ u32 s_hist[LZE_SYMS];
    const u32 tid = threadIdx.x, A = 32 + in.o;
    for (u32 j = tid; j < LZE_SYMS; j += PFB_THREADS) s_hist[j] = 0;
    __syncthreads();
    const u64 step = (u64)gridDim.x * PFB_THREADS, first = (u64)blockIdx.x * PFB_THREADS + tid;
    u32 bad = 0;
    for (u32 f = 0; f < 3; ++f) {
        const u32 *row = lzw_row(in, f);
        for (u64 k = first; k < in.n_seq; k += step) {
            u32 log, res;
            const u32 b = lze_bin(row[k], in.o, &log, &res);
            if (b < A) atomicAdd(&s_hist[f * LZE_FIELD_K + b], 1u);
            else bad = 1;
        }
    }
    for (u64 k = first; k < in.n_lit; k += step) atomicAdd(&s_hist[LZE_LIT_BASE + in.lit[k]], 1u);
    __syncthreads();
    for (u32 j = tid; j < LZE_SYMS; j += PFB_THREADS)
        if (s_hist[j]) atomicAdd(&sc.hist[j], s_hist[j]);
    if (bad) atomicOr(&sc.head->flags, (u32)SCL_ST_SYMBOL);
}

// ONE workgroup: trees, code tables, sizes, positions, faults -- scl_lz77_entropy.hip's order of decisions
__global__ void __launch_bounds__(PFB_THREADS) lzw_layout_kernel(LzwEncIn in, LzwEncScratch sc, u64 out_cap_bytes,
                                                                 u64 *__restrict__ nbits_out, u32 *__restrict__ status_out) {
    __shared__ u32 hist[LZE_SYMS], code[LZE_SYMS];
    __shared__ u8 clen[LZE_SYMS];
    __shared__ LzeSmallTree small[3];
    __shared__ LzeBigTree big;
    __shared__ u32 n_leaves[4], flags;
    __shared__ u64 s_wave[PFB_THREADS / 64];
    const u32 tid = threadIdx.x, o = in.o, A = 32 + o;
    for (u32 j = tid; j < LZE_SYMS; j += PFB_THREADS) {
        hist[j] = sc.hist[j];
        code[j] = 0;
        clen[j] = 0;
    }
    if (tid == 0) flags = sc.head->flags;
    __syncthreads();
    lze_build_codes<PFB_THREADS>(hist, A, tid, small, big, n_leaves, code, clen, &flags);
    u32 status = flags;
    u64 pos = 0;
    bool header_overflow = false;
    for (u32 f = 0; f < 4; ++f) {
        const u32 base = f * LZE_FIELD_K, K = f < 3 ? A : 256u, n = f < 3 ? in.n_seq : in.n_lit;
        u64 cs = 0, vs = 0, rs = 0;
        if (n && status == 0) {  // (uniform)
            u64 c_cs = 0, c_vs = 0, c_rs = 0;
            if (tid < K) {
                const u32 c = hist[base + tid];
                u64 val;
                c_cs = lze_elias_delta(c, &val);
                if (c) c_vs = (u64)c * clen[base + tid];
                if (f < 3 && tid >= o) c_rs = (u64)c * (tid - o);
            }
            (void)scl_block_scan_excl<u64, PFB_THREADS, SclScanSum>(c_cs, s_wave, &cs);
            (void)scl_block_scan_excl<u64, PFB_THREADS, SclScanSum>(c_vs, s_wave, &vs);
            (void)scl_block_scan_excl<u64, PFB_THREADS, SclScanSum>(c_rs, s_wave, &rs);
        }
        if (vs >> 32) header_overflow = true;  // does not fit its own header
        if (tid == 0) {
            sc.head->field_at[f] = pos;
            sc.head->counts_size[f] = (u32)cs;
            sc.head->values_size[f] = (u32)vs;
            const u64 values_at = pos + 64 + cs;
            if (f < 3) {
                sc.head->section_at[2 * f] = values_at;
                sc.head->section_at[2 * f + 1] = values_at + vs;
            } else {
                sc.head->section_at[6] = values_at;
            }
        }
        pos += n ? 64 + cs + vs + rs : 32;
    }
    if (status) pos = 0;
    else if (header_overflow || (pos + 7) / 8 > out_cap_bytes) status = SCL_ST_CAPACITY;
    for (u32 j = tid; j < LZE_SYMS; j += PFB_THREADS) sc.enc[j] = make_uint2(code[j], clen[j]);
    if (tid == 0) {
        sc.head->total_bits = pos;
        sc.head->tile.fits = status == 0 ? 1u : 0u;
        *nbits_out = pos;
        *status_out = status;
    }
}

__global__ void __launch_bounds__(PFB_THREADS) lzw_zero_kernel(const LzwEncHead *__restrict__ head, u32 *__restrict__ out32,
                                                               u64 tail_index) {
    if (!head->tile.fits) return;
    const u64 n_words = (head->total_bits + 31) >> 5;  // all of them inside out_cap_bytes but, maybe, the tail word
    for (u64 w = (u64)blockIdx.x * PFB_THREADS + threadIdx.x; w < n_words; w += (u64)gridDim.x * PFB_THREADS)
        if (w != tail_index) out32[w] = 0;
}

// the low `len` <= 43 bits of val, most significant first, at bit `at` of the zeroed output
__device__ __forceinline__ void lzw_or_bits(LzwEncHead *head, u32 *out32, u64 tail_index, u64 at, u64 val, u32 len) {
    if (len == 0) return;
    const u64 w = at >> 5;
    const u32 sh = (u32)(at & 31);
    const u64 top = val << (64 - len);
    const u64 t = top >> sh;
    const u32 part[3] = {(u32)(t >> 32), (u32)t, sh ? (u32)((top << (64 - sh)) >> 32) : 0u};
#pragma unroll
    for (u32 i = 0; i < 3; ++i)
        if (part[i]) atomicOr(w + i == tail_index ? &head->tile.tail_word : out32 + w + i, scl_bswap32(part[i]));
}

// one workgroup per field: [counts_size][the counts][values_size]
__global__ void __launch_bounds__(PFB_THREADS) lzw_heads_kernel(LzwEncIn in, LzwEncScratch sc, u32 *__restrict__ out32,
                                                                u64 tail_index) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    LzwEncHead *head = sc.head;
    if (!head->tile.fits) return;
    const u32 f = blockIdx.x, tid = threadIdx.x;
    const u32 K = f < 3 ? 32 + in.o : 256u, n = f < 3 ? in.n_seq : in.n_lit;
    if (n == 0) return;  // one zero header
    u64 val = 0;
    u32 len = 0, total;
    if (tid < K) len = lze_elias_delta(sc.hist[f * LZE_FIELD_K + tid], &val);
    const u32 off = scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(len, s_wave, &total);
    const u64 at = head->field_at[f];
    lzw_or_bits(head, out32, tail_index, at + 32 + off, val, len);
    if (tid == 0) {
        lzw_or_bits(head, out32, tail_index, at, head->counts_size[f], 32);
        lzw_or_bits(head, out32, tail_index, at + 32 + total, head->values_size[f], 32);
    }
}

// the value policy of pfb_tile_bits_body / pfb_encode_tile_body: the code tables of lzw_layout, from scratch into LDS.  No
// fault is raised here: lzw_hist found the values without a bin.
struct LzwEnc {
    const LzwEncIn &in;
    const LzwEncScratch &sc;
    u32 seq_tiles;
    uint2 *s_enc;  // [LZE_SYMS]
    u32 section;   // of the tile that codes() loaded
    static constexpr bool kTables = true;
    static constexpr u32 kFault = 0;

    __device__ __forceinline__ void load() const {
        for (u32 j = threadIdx.x; j < LZE_SYMS; j += PFB_THREADS) s_enc[j] = sc.enc[j];
    }
    __device__ __forceinline__ u64 tile_base(u32 block) const { return sc.head->section_at[section] + sc.tile_bits[block]; }
    // the {bits, length} of the thread's PFB_PER_THREAD consecutive values of tile `block` of the seven sections
    __device__ __forceinline__ u32 codes(u32 block, uint2 (&e)[PFB_PER_THREAD], u32 &) {
        const u32 s = block < 6 * seq_tiles ? block / seq_tiles : 6u;
        const u32 tile = s < 6 ? block - s * seq_tiles : block - 6 * seq_tiles;
        const u64 first = (u64)tile * PFB_TILE + threadIdx.x * PFB_PER_THREAD;
        section = s;
        u32 bits = 0;
        if (s < 6) {
            const u32 f = s >> 1;
            const u32 *row = lzw_row(in, f);
#pragma unroll
            for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
                uint2 c = make_uint2(0u, 0u);
                if (first + j < in.n_seq) {
                    u32 log, res;
                    const u32 b = lze_bin(row[first + j], in.o, &log, &res);
                    c = (s & 1u) ? make_uint2(res, log) : s_enc[f * LZE_FIELD_K + b];
                }
                e[j] = c;
                bits += c.y;
            }
        } else {
#pragma unroll
            for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
                const uint2 c = first + j < in.n_lit ? s_enc[LZE_LIT_BASE + in.lit[first + j]] : make_uint2(0u, 0u);
                e[j] = c;
                bits += c.y;
            }
        }
        return bits;
    }
};

__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_tile_bits_kernel(LzwEncIn in, LzwEncScratch sc, u32 seq_tiles) {
    __shared__ uint2 s_enc[LZE_SYMS];
    if (!sc.head->tile.fits) return;  // (uniform: the whole grid leaves)
    pfb_tile_bits_body(LzwEnc{in, sc, seq_tiles, s_enc, 0u}, sc.tile_bits, (u32 *)nullptr);
}

// ONE workgroup: the tile sums of every section become the tile offsets inside it
__global__ void __launch_bounds__(PFB_SCAN_THREADS) lzw_scan_tiles_kernel(LzwEncScratch sc, u32 seq_tiles, u32 lit_tiles) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    if (!sc.head->tile.fits) return;
    for (u32 s = 0; s < LZW_SECTIONS; ++s)
        (void)scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(sc.tile_bits + (u64)s * seq_tiles, s < 6 ? seq_tiles : lit_tiles,
                                                                      s_wave);
}

__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_emit_kernel(LzwEncIn in, LzwEncScratch sc, u32 seq_tiles,
                                                                  u32 *__restrict__ out32, u64 tail_index) {
    __shared__ uint2 s_enc[LZE_SYMS];
    pfb_encode_tile_body(LzwEnc{in, sc, seq_tiles, s_enc, 0u}, &sc.head->tile, out32, tail_index);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
struct LzwDecState {   // head of the decoder's scratch (256 bytes, zeroed by the entry point); the host reads it per field
    PfbDecHead sync;   // first: the host reads its two pass words from byte 0; n_total and last_group are of the section
    u64 pos;           // bits of the stream used so far: `consumed`
    u32 status, go;    // go: the field has a values section to decode (lzw_dec_head)
    u32 count[4];      // values decoded per field
    u64 values_at;     // the section's first bit, relative to the stream
    u32 values_size, m;  // its bits; the leaves of its tree
    u64 resid_total;   // lzw_resid_scan
    u64 resid_fail_at;   // lzw_resid: the residual bits in front of the first step of 64 values that in_nbits cuts
    u32 resid_fail_k;    //            that step's first value
    u32 resid_overflow;  //            the first value that no 32-bit field holds
    u32 resid_pending, pad;
};

struct LzwDecScratch {
    LzwDecState *state;
    u32 *lut;          // [LZW_LUT_SIZE]
    u16 *kids;         // [2 * LZ_HUFF_MAX_K]
    u16 *leaf_sym;     // [LZ_HUFF_MAX_K]
    u64 *resid_bits;   // [tiles(seq_cap)]
    PfbDecGroups g;    // positions relative to the section; a section ends with PFB_END_STATE only
};

struct LzwDecIn {
    const u8 *in;
    u64 in_size_bytes, in_bit_offset, in_nbits;
    u32 o;
};

// what the residuals of the field before left to decide: the one-lane decoder stops at the first step of 64 values that the
// input cuts (SCL_ST_TRUNCATED, the steps before it count as consumed) and reports a value above 2^32 - 1 met until then
__device__ __forceinline__ void lzw_field_end(LzwDecState *S) {
    if (!S->resid_pending) return;
    S->resid_pending = 0;
    u32 st = 0;
    if (S->resid_fail_k != LZW_NONE32) {
        st |= SCL_ST_TRUNCATED;
        S->pos += S->resid_fail_at;
    } else {
        S->pos += S->resid_total;
    }
    if (S->resid_overflow < S->resid_fail_k) st |= SCL_ST_STATE;
    S->status = st;
}

// ONE workgroup: the headers, the counts and the tree of field f, as lz77_entropy_decode reads them
__global__ void __launch_bounds__(PFB_THREADS) lzw_dec_head_kernel(LzwDecIn a, LzwDecScratch sc, u32 f) {
    __shared__ u32 hist[LZ_HUFF_MAX_K];
    __shared__ LzeBigTree tree;
    __shared__ u32 sh_m, sh_status, sh_go, sh_values_size;
    __shared__ u64 sh_pos;
    const u32 tid = threadIdx.x;
    const u32 K = f < 3 ? 32 + a.o : 256u;
    LzwDecState *S = sc.state;
    hist[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        lzw_field_end(S);
        u32 st = S->status, go = 0, values_size = 0, m = 0;
        u64 pos = S->pos;
        const u64 at = a.in_bit_offset, nbits = a.in_nbits;
        if (st == 0) do {
            if (pos + 32 > nbits) {
                st = SCL_ST_TRUNCATED;
                break;
            }
            const u32 counts_size = lze_read_bits(a.in, at + pos, 32);
            pos += 32;
            if (counts_size == 0) break;  // a field without values
            if (pos + counts_size > nbits) {
                st = SCL_ST_TRUNCATED;
                break;
            }
            st = lze_parse_counts(a.in, at + pos, counts_size, K, hist);
            if (st) break;
            pos += counts_size;
            if (pos + 32 > nbits) {
                st = SCL_ST_TRUNCATED;
                break;
            }
            values_size = lze_read_bits(a.in, at + pos, 32);
            pos += 32;
            if (pos + values_size > nbits) {
                st = SCL_ST_TRUNCATED;
                break;
            }
            const LzHuffTree t = {tree.prob, tree.heap, tree.parent, tree.kids, tree.leaf_sym};
            m = lz_huffman_build(hist, K, t);
            go = 1;
        } while (0);
        sh_m = m;
        sh_status = st;
        sh_go = go;
        sh_values_size = values_size;
        sh_pos = pos;
    }
    __syncthreads();
    const u32 m = sh_m, go = sh_go;
    if (go) {  // (uniform)
        for (u32 i = tid; i < m; i += PFB_THREADS) {
            u32 c;
            if (lz_huffman_leaf_code(tree.parent, i, &c) > LZ_HUFF_MAX_CODE_BITS) atomicOr(&sh_status, (u32)SCL_ST_SIZE);
        }
        __syncthreads();
    }
    const u32 status = sh_status;
    if (go && status == 0) {
        const u32 root = lz_huffman_root(m);
        for (u32 p = tid; p < LZW_LUT_SIZE; p += PFB_THREADS) {
            u32 node = root, entry = (LZW_KIND_NODE << 30) | (LZW_LUT_BITS << 16);
            for (u32 d = 0; d < LZW_LUT_BITS; ++d) {
                const u32 child = tree.kids[2 * (node - m) + ((p >> (LZW_LUT_BITS - 1 - d)) & 1u)];
                if (child == LZ_HUFF_NONE) {
                    entry = (LZW_KIND_NONE << 30) | ((d + 1) << 16);
                    break;
                }
                if (child < m) {
                    entry = (LZW_KIND_LEAF << 30) | ((d + 1) << 16) | tree.leaf_sym[child];
                    break;
                }
                node = child;
            }
            if ((entry >> 30) == LZW_KIND_NODE) entry |= node;
            sc.lut[p] = entry;
        }
        for (u32 i = tid; i < 2 * LZ_HUFF_MAX_K; i += PFB_THREADS) sc.kids[i] = i < 2 * m ? tree.kids[i] : (u16)LZ_HUFF_NONE;
        sc.leaf_sym[tid] = tid < m ? tree.leaf_sym[tid] : (u16)0;
    }
    if (tid == 0) {
        S->status = status;
        S->pos = sh_pos;
        S->go = go && status == 0 && sh_values_size ? 1u : 0u;
        S->count[f] = 0;
        S->values_at = sh_pos;
        S->values_size = sh_values_size;
        S->m = m;
        S->sync.start_pass = S->sync.exit_pass = 0;
        S->resid_total = 0;
        S->resid_fail_at = PFB_NONE64;
        S->resid_fail_k = S->resid_overflow = LZW_NONE32;
    }
}

// the codeword policy of pfb_sync_body / pfb_write_body: the tree of the field, from scratch into LDS
struct LzwCode {
    const LzwDecScratch &sc;  // lzw_dec_head's lut, kids and leaf_sym
    u32 *s_lut;             // [LZW_LUT_SIZE]
    u16 *s_kids, *s_leaf;   // [2 * LZ_HUFF_MAX_K], [LZ_HUFF_MAX_K]
    u32 m;

    __device__ __forceinline__ void load() const {
        for (u32 i = threadIdx.x; i < LZW_LUT_SIZE; i += PFB_THREADS) s_lut[i] = sc.lut[i];
        for (u32 i = threadIdx.x; i < 2 * LZ_HUFF_MAX_K; i += PFB_THREADS) s_kids[i] = sc.kids[i];
        for (u32 i = threadIdx.x; i < LZ_HUFF_MAX_K; i += PFB_THREADS) s_leaf[i] = sc.leaf_sym[i];
    }
    __device__ __forceinline__ u32 len_gcd() const { return 1u; }  // (no gcd is kept for a tree built on the device)
    // PFB_END_EXIT: a symbol of `len` bits; PFB_END_STATE: what ends the one-lane walk -- a bit into the missing child, or the
    // section cut the codeword.
    __device__ __forceinline__ u32 codeword(u32 bits, u32 rem, u32 &len, u32 &sym) const {
        const u32 e = s_lut[bits >> (32u - LZW_LUT_BITS)];
        const u32 kind = e >> 30;
        len = (e >> 16) & 63u;
        sym = e & 0xFFFFu;
        if (len > rem) return PFB_END_STATE;
        if (kind == LZW_KIND_LEAF) return PFB_END_EXIT;
        if (kind == LZW_KIND_NONE) return PFB_END_STATE;
        u32 node = sym;
        for (u32 d = LZW_LUT_BITS; d < LZ_HUFF_MAX_CODE_BITS; ++d) {
            if (d == rem) return PFB_END_STATE;
            const u32 next = s_kids[2 * (node - m) + ((bits >> (31u - d)) & 1u)];
            if (next == LZ_HUFF_NONE) return PFB_END_STATE;
            if (next < m) {
                sym = s_leaf[next];
                len = d + 1;
                return PFB_END_EXIT;
            }
            node = next;
        }
        return PFB_END_STATE;  // (not reached: lzw_dec_head refused a code above 32 bits)
    }
};

// the field's section: `base_bit` = its first bit in the input, `nbits` = values_size
__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_sync_kernel(LzwDecIn a, u64 base_bit, u64 nbits, u64 n_sub, u64 n_groups,
                                                                  LzwDecScratch sc, u32 m, u32 pass) {
    __shared__ u32 s_lut[LZW_LUT_SIZE];
    __shared__ u16 s_kids[2 * LZ_HUFF_MAX_K], s_leaf[LZ_HUFF_MAX_K];
    pfb_sync_body(LzwCode{sc, s_lut, s_kids, s_leaf, m}, a.in, a.in_size_bytes, base_bit, nbits, n_sub, n_groups, &sc.state->sync,
                  sc.g, pass);
}

// ONE workgroup: where the section ends, the symbol offsets of the workgroups up to there, the field's count and status as
// the one-lane walk decides them: more symbols than `cap` is SCL_ST_CAPACITY at the leaf behind the cap, before any later
// fault; otherwise a cut is SCL_ST_STATE
__global__ void __launch_bounds__(PFB_SCAN_THREADS) lzw_scan_groups_kernel(LzwDecScratch sc, u64 n_groups, u64 cap, u32 f) {
    u64 total;
    const u64 last_group = pfb_scan_to_end(sc.g, n_groups, &total);
    if (threadIdx.x == 0) {
        LzwDecState *S = sc.state;
        const u64 cut = sc.g.group_end[last_group];
        u32 status = 0;
        if (total > cap) status = SCL_ST_CAPACITY;
        else if (cut != PFB_NONE64) status = SCL_ST_STATE;
        S->sync.n_total = total;
        S->sync.last_group = last_group;
        S->count[f] = (u32)(total < cap ? total : cap);
        S->status = status;
        if (status == 0) {
            S->pos += S->values_size;
            S->resid_pending = f < 3 ? 1u : 0u;
        }
    }
}

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_write_kernel(LzwDecIn a, u64 base_bit, u64 nbits, u64 n_sub,
                                                                   LzwDecScratch sc, u32 m, SYM *__restrict__ out, u64 cap) {
    __shared__ u32 s_lut[LZW_LUT_SIZE];
    __shared__ u16 s_kids[2 * LZ_HUFF_MAX_K], s_leaf[LZ_HUFF_MAX_K];
    pfb_write_body(LzwCode{sc, s_lut, s_kids, s_leaf, m}, a.in, a.in_size_bytes, base_bit, nbits, n_sub, &sc.state->sync, sc.g, out,
                   cap, (u64 *)nullptr);
}

// the residual width of the thread's PFB_PER_THREAD consecutive bins of tile `tile` (0 past the field's count)
__device__ __forceinline__ u32 lzw_resid_widths(const u32 *row, u64 n, u32 o, u64 first, u32 (&b)[PFB_PER_THREAD]) {
    u32 bits = 0;
#pragma unroll
    for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
        b[j] = first + j < n ? row[first + j] : 0u;
        if (first + j < n && b[j] >= o) bits += b[j] - o;
    }
    return bits;
}

__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_resid_bits_kernel(LzwDecScratch sc, const u32 *__restrict__ row, u32 o,
                                                                        u32 f) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    const LzwDecState *S = sc.state;
    if (S->status) return;  // (uniform)
    u32 b[PFB_PER_THREAD], total;
    const u32 bits = lzw_resid_widths(row, S->count[f], o, (u64)blockIdx.x * PFB_TILE + threadIdx.x * PFB_PER_THREAD, b);
    (void)scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &total);
    if (threadIdx.x == 0) sc.resid_bits[blockIdx.x] = total;
}

__global__ void __launch_bounds__(PFB_SCAN_THREADS) lzw_resid_scan_kernel(LzwDecScratch sc, u64 n_tiles) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    if (sc.state->status) return;
    const u64 total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(sc.resid_bits, n_tiles, s_wave);
    if (threadIdx.x == 0) sc.state->resid_total = total;
}

// bins -> values, in place.  A value whose bits the input cuts marks its step of 64 values (four threads); nothing of such a
// step needs storing, and no bit at or past in_nbits is read.
__global__ void __launch_bounds__(PFB_THREADS, 4) lzw_resid_kernel(LzwDecIn a, LzwDecScratch sc, u32 *__restrict__ row, u32 f) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_off[PFB_THREADS];
    LzwDecState *S = sc.state;
    if (S->status) return;  // (uniform)
    const u32 tid = threadIdx.x, o = a.o;
    const u64 n = S->count[f], first = (u64)blockIdx.x * PFB_TILE + tid * PFB_PER_THREAD;
    if ((u64)blockIdx.x * PFB_TILE >= n) return;  // (uniform)
    const u64 section = S->pos;                   // the residuals' first bit, relative to the stream
    const u64 avail = a.in_nbits - section;
    u32 b[PFB_PER_THREAD], total;
    const u32 bits = lzw_resid_widths(row, n, o, first, b);
    const u32 mine = scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &total);
    s_off[tid] = mine;
    __syncthreads();
    const u64 tile_off = sc.resid_bits[blockIdx.x];
    u64 off = tile_off + mine;
    bool cut = false;
    u32 overflow = LZW_NONE32;
#pragma unroll
    for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
        if (first + j >= n || b[j] < o) continue;
        const u32 log = b[j] - o;
        if (off + log > avail) {
            cut = true;
            break;
        }
        const u64 v = (u64)o + (1ull << log) + lze_read_bits(a.in, a.in_bit_offset + section + off, log) - 1;
        if (v >> 32) overflow = min(overflow, (u32)(first + j));
        else row[first + j] = (u32)v;
        off += log;
    }
    if (cut) {
        atomicMin((unsigned long long *)&S->resid_fail_at, (unsigned long long)(tile_off + s_off[tid & ~3u]));
        atomicMin(&S->resid_fail_k, (u32)(first & ~63ull));
    }
    if (overflow != LZW_NONE32) atomicMin(&S->resid_overflow, overflow);
}

__global__ void lzw_finish_kernel(LzwDecScratch sc, u32 sync_passes, scl_lz77_entropy_wide_result *__restrict__ result) {
    LzwDecState *S = sc.state;
    lzw_field_end(S);
    const u32 c0 = S->count[0], c1 = S->count[1], c2 = S->count[2];
    const u32 n_seq = min(c0, min(c1, c2));
    u32 status = S->status;
    if (status == 0 && (c0 != n_seq || c1 != n_seq || c2 != n_seq)) status = SCL_ST_STATE;
    result->consumed = S->pos;
    result->n_seq = n_seq;
    result->n_lit = S->count[3];
    result->status = status;
    result->sync_passes = sync_passes;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct LzwEncLayout {
    u64 head, hist, enc, tile_bits, total;
};
LzwEncLayout lzw_enc_layout(u64 n_seq, u64 n_lit) {
    LzwEncLayout l;
    SclCarver c;
    l.head = c.take(sizeof(LzwEncHead));
    l.hist = c.take(LZE_SYMS * 4);
    l.enc = c.take(LZE_SYMS * 8);
    l.tile_bits = c.take((6 * pfb_tiles(n_seq) + pfb_tiles(n_lit)) * 8);
    l.total = c.at;
    return l;
}

struct LzwDecLayout {
    u64 state, lut, kids, leaf_sym, resid_bits, group_exit, group_count, group_end, sub, total;
};
LzwDecLayout lzw_dec_layout(u64 seq_cap, u64 in_nbits) {
    const u64 g = pfb_groups(in_nbits);
    LzwDecLayout l;
    SclCarver c;
    l.state = c.take(sizeof(LzwDecState));
    l.lut = c.take(LZW_LUT_SIZE * 4);
    l.kids = c.take(2 * LZ_HUFF_MAX_K * 2);
    l.leaf_sym = c.take(LZ_HUFF_MAX_K * 2);
    l.resid_bits = c.take(pfb_tiles(seq_cap) * 8);
    l.group_exit = c.take(2 * g * 8);
    l.group_count = c.take(g * 8);
    l.group_end = c.take(g * 8);
    l.sub = c.take(g * PFB_THREADS * 4);
    l.total = c.at;
    return l;
}

static_assert(sizeof(LzwEncHead) <= 256 && sizeof(LzwDecState) <= 256, "the heads are one carved part each");
static_assert(offsetof(LzwDecState, sync) == 0, "the host reads the two pass words from byte 0 of the scratch");

}  // namespace

extern "C" uint64_t scl_lz77_entropy_wide_scratch_bytes(uint64_t n_seq, uint64_t n_lit, uint64_t in_nbits) {
    const u64 e = lzw_enc_layout(n_seq, n_lit).total, d = lzw_dec_layout(n_seq, in_nbits).total;
    return e > d ? e : d;
}

// In coded values, 3 * n_seq + n_lit.  Set from the sweep of tools/bench_lz77.py --wide (profiles/lz77_bench.txt, DESIGN.md
// 3.6.3): the smallest measured stream from which both wide calls beat the one-wave kernels at every larger measured stream
// on both sources -- 64 KiB of the Markov source, 5239 sequences and 32548 literals.  The streams of the all-equal source
// (9 values at every block size) lie below it and lose.
extern "C" uint64_t scl_lz77_entropy_wide_threshold(void) { return 3ull * 5239 + 32548; }

extern "C" int scl_lz77_entropy_wide_kernel_names(char *emit, char *sync, char *resid, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_entropy_wide_kernel_names: cap must be at least 96");
    if (emit) snprintf(emit, cap, "lzw_emit_kernel");
    if (sync) snprintf(sync, cap, "lzw_sync_kernel");
    if (resid) snprintf(resid, cap, "lzw_resid_kernel");
    return SCL_OK;
}

extern "C" int scl_lz77_entropy_encode_wide(const scl_lz77_entropy_wide_encode_args *a, void *stream) {
    const char *what = "lz77_entropy_encode_wide";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_out && a->d_nbits && a->d_status && a->d_scratch && (a->n_lit == 0 || a->d_literals) &&
                    (a->n_seq == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->binned_offset <= 32, "%s: binned_offset %u: 0 <= binned_offset <= 32", what, a->binned_offset);
    SCL_REQUIRE(a->n_seq < (1ull << 32) && a->n_lit < (1ull << 32), "%s: a stream holds fewer than 2^32 sequences and literals",
                what);
    SCL_REQUIRE((((uintptr_t)a->d_out | (uintptr_t)a->d_lit_count | (uintptr_t)a->d_match_len | (uintptr_t)a->d_match_off) & 3) == 0 &&
                    (((uintptr_t)a->d_scratch | (uintptr_t)a->d_nbits) & 7) == 0,
                "%s: d_out and the rows must be 4-byte, d_scratch and d_nbits 8-byte aligned", what);
    const LzwEncLayout l = lzw_enc_layout(a->n_seq, a->n_lit);
    SCL_REQUIRE(a->scratch_bytes >= l.total, "%s: scratch of %llu bytes, scl_lz77_entropy_wide_scratch_bytes asks for %llu", what,
                (unsigned long long)a->scratch_bytes, (unsigned long long)l.total);
    hipStream_t st = (hipStream_t)stream;
    u8 *p = (u8 *)a->d_scratch;
    const LzwEncScratch sc = {(LzwEncHead *)(p + l.head), (u32 *)(p + l.hist), (uint2 *)(p + l.enc), (u64 *)(p + l.tile_bits)};
    const LzwEncIn in = {{a->d_lit_count, a->d_match_len, a->d_match_off}, a->d_literals, (u32)a->n_seq, (u32)a->n_lit,
                         a->binned_offset};
    SCL_HIP_TRY(hipMemsetAsync(p, 0, l.enc, st));  // the head and the histograms
    const u64 seq_tiles = pfb_tiles(a->n_seq), lit_tiles = pfb_tiles(a->n_lit), n_tiles = 6 * seq_tiles + lit_tiles;
    const u64 most = seq_tiles > lit_tiles ? seq_tiles : lit_tiles;
    const u32 hist_grid = (u32)(most * PFB_PER_THREAD < LZW_HIST_MAX_GRID ? (most ? most * PFB_PER_THREAD : 1) : LZW_HIST_MAX_GRID);
    hipLaunchKernelGGL(lzw_hist_kernel, dim3(hist_grid), dim3(PFB_THREADS), 0, st, in, sc);
    hipLaunchKernelGGL(lzw_layout_kernel, dim3(1), dim3(PFB_THREADS), 0, st, in, sc, a->out_cap_bytes, a->d_nbits, a->d_status);
    const u64 tail_index = (a->out_cap_bytes & 3) ? a->out_cap_bytes >> 2 : PFB_NONE64;
    u32 *out32 = (u32 *)a->d_out;
    const u64 cap_words = (a->out_cap_bytes + 3) >> 2;
    if (cap_words) {
        const u64 zero_blocks = (cap_words + PFB_THREADS - 1) / PFB_THREADS;
        hipLaunchKernelGGL(lzw_zero_kernel, dim3((u32)(zero_blocks < LZW_ZERO_MAX_GRID ? zero_blocks : LZW_ZERO_MAX_GRID)),
                           dim3(PFB_THREADS), 0, st, (const LzwEncHead *)sc.head, out32, tail_index);
        hipLaunchKernelGGL(lzw_heads_kernel, dim3(4), dim3(PFB_THREADS), 0, st, in, sc, out32, tail_index);
        if (n_tiles) {
            hipLaunchKernelGGL(lzw_tile_bits_kernel, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, in, sc, (u32)seq_tiles);
            hipLaunchKernelGGL(lzw_scan_tiles_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, (u32)seq_tiles, (u32)lit_tiles);
            hipLaunchKernelGGL(lzw_emit_kernel, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, in, sc, (u32)seq_tiles, out32,
                               tail_index);
        }
        if (a->out_cap_bytes & 3)
            hipLaunchKernelGGL(pfb_encode_tail_kernel, dim3(1), dim3(1), 0, st, (const PfbEncScratch *)&sc.head->tile,
                               (const u64 *)&sc.head->total_bits, a->d_out, a->out_cap_bytes);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_lz77_entropy_decode_wide(const scl_lz77_entropy_wide_decode_args *a, void *stream) {
    const char *what = "lz77_entropy_decode_wide";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_result && a->d_scratch && (a->in_size_bytes == 0 || a->d_in) && (a->lit_cap == 0 || a->d_literals) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->binned_offset <= 32, "%s: binned_offset %u: 0 <= binned_offset <= 32", what, a->binned_offset);
    SCL_REQUIRE(a->seq_cap < (1ull << 32) && a->lit_cap < (1ull << 32), "%s: a stream holds fewer than 2^32 sequences and literals",
                what);
    SCL_REQUIRE(a->in_nbits < (1ull << 46) && a->in_bit_offset < (1ull << 62), "%s: stream of %llu bits: 2^46 and more are not coded",
                what, (unsigned long long)a->in_nbits);
    SCL_REQUIRE((a->in_bit_offset + a->in_nbits + 7) / 8 <= a->in_size_bytes, "%s: the stream ends behind in_size_bytes", what);
    SCL_REQUIRE((((uintptr_t)a->d_in | (uintptr_t)a->d_lit_count | (uintptr_t)a->d_match_len | (uintptr_t)a->d_match_off) & 3) == 0 &&
                    (((uintptr_t)a->d_scratch | (uintptr_t)a->d_result) & 7) == 0,
                "%s: d_in and the rows must be 4-byte, d_scratch and d_result 8-byte aligned", what);
    const LzwDecLayout l = lzw_dec_layout(a->seq_cap, a->in_nbits);
    SCL_REQUIRE(a->scratch_bytes >= l.total, "%s: scratch of %llu bytes, scl_lz77_entropy_wide_scratch_bytes asks for %llu", what,
                (unsigned long long)a->scratch_bytes, (unsigned long long)l.total);
    hipStream_t st = (hipStream_t)stream;
    u8 *p = (u8 *)a->d_scratch;
    const LzwDecScratch sc = {(LzwDecState *)(p + l.state), (u32 *)(p + l.lut), (u16 *)(p + l.kids), (u16 *)(p + l.leaf_sym),
                              (u64 *)(p + l.resid_bits),
                              {(u32 *)(p + l.sub), (u64 *)(p + l.group_exit), (u64 *)(p + l.group_count), (u64 *)(p + l.group_end)}};
    const LzwDecIn in = {a->d_in, a->in_size_bytes, a->in_bit_offset, a->in_nbits, a->binned_offset};
    SCL_HIP_TRY(hipMemsetAsync(sc.state, 0, sizeof(LzwDecState), st));
    u32 sync_passes = 0;
    for (u32 f = 0; f < 4; ++f) {
        hipLaunchKernelGGL(lzw_dec_head_kernel, dim3(1), dim3(PFB_THREADS), 0, st, in, sc, f);
        SCL_HIP_TRY(hipGetLastError());
        LzwDecState h;
        SCL_HIP_TRY(hipMemcpyAsync(&h, sc.state, sizeof(h), hipMemcpyDeviceToHost, st));
        SCL_HIP_TRY(hipStreamSynchronize(st));
        if (h.status) break;
        if (!h.go) continue;
        const u64 nbits = h.values_size, base_bit = a->in_bit_offset + h.values_at;
        const u64 cap = f < 3 ? a->seq_cap : a->lit_cap;
        u32 *row = f == 0 ? a->d_lit_count : f == 1 ? a->d_match_len : a->d_match_off;
        const dim3 block(PFB_THREADS);
        const auto sync = [&](dim3 grid, u64 n_sub, u64 n_groups, u32 pass) {
            hipLaunchKernelGGL(lzw_sync_kernel, grid, block, 0, st, in, base_bit, nbits, n_sub, n_groups, sc, h.m, pass);
        };
        const auto scan = [&](u64 n_groups, u32) {
            hipLaunchKernelGGL(lzw_scan_groups_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, n_groups, cap, f);
        };
        const auto write = [&](dim3 grid, u64 n_sub) {
            if (f < 3) hipLaunchKernelGGL(lzw_write_kernel<u32>, grid, block, 0, st, in, base_bit, nbits, n_sub, sc, h.m, row, cap);
            else hipLaunchKernelGGL(lzw_write_kernel<u8>, grid, block, 0, st, in, base_bit, nbits, n_sub, sc, h.m, a->d_literals, cap);
        };
        if (int rc = pfb_decode_section(nbits, sc.state, st, &sync_passes, sync, scan, write)) return rc;
        // the bins become values.  A codeword has at least one bit: the section holds at most `nbits` values
        const u64 n_tiles = f < 3 ? pfb_tiles(cap < nbits ? cap : nbits) : 0;
        if (n_tiles) {
            hipLaunchKernelGGL(lzw_resid_bits_kernel, dim3((u32)n_tiles), block, 0, st, sc, (const u32 *)row, a->binned_offset, f);
            hipLaunchKernelGGL(lzw_resid_scan_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, n_tiles);
            hipLaunchKernelGGL(lzw_resid_kernel, dim3((u32)n_tiles), block, 0, st, in, sc, row, f);
        }
        SCL_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lzw_finish_kernel, dim3(1), dim3(1), 0, st, sc, sync_passes, a->d_result);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}
