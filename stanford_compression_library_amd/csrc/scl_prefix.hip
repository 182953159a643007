// scl_prefix.hip -- batched prefix-free (Huffman, ...) coding for gfx950, one wavefront lane per chunk.
//
// Replaces reference scl/compressors/prefix_free_compressors.py:
//   PrefixFreeEncoder.encode_block :31-50  the codewords of the block back to back: no size header, no terminator
//   PrefixFreeDecoder.decode_block :67-88  walks the code tree from bit 0 until every bit of the stream is consumed
// and serves any prefix-free code table (HuffmanTree, huffman_coder.py:45-93, is built on the host by the Python class).
// Stream layout per chunk: [codeword of symbol 0][codeword of symbol 1]...  -- nbits = sum of the code lengths, 0 for an
// empty chunk.  Streams grow front to back: bit_offset[c] = 8 * c * out_stride.
//
// Two forms, as for every coder:
//   tuned (byte symbols, K <= 256)
//     encode: {code, len} table in LDS (2 KiB), 128-byte symbol lines in registers, one put_field per symbol into the
//             bounded forward lane writer of scl_ans_fast_io.h (AnsFwdWriter<.., BOUNDED>): whole 128-byte lines out.
//     decode: the next T = min(max_len, 11) bits index a table of 2^T 16-bit entries in LDS (<= 4 KiB); an entry is a
//             (symbol, len), or the tree node the walk continues from bit by bit (codes longer than T), or "no such
//             code" with the depth at which an incomplete tree ends.  The nodes below depth T (<= 512, 2 KiB) sit in
//             LDS too, so one kernel serves every length up to 32.  Input through AnsBitReader's LDS word ring (whole
//             128-byte lines in); decoded symbols leave as whole 16-byte pieces, the last partial piece byte by byte.
//             32 KiB ring + 4 KiB + 2 KiB = 38 KiB per workgroup: four workgroups per CU.
//   any-parameter (symbol type a template parameter, K <= 65536): tables read where they are in device memory, a plain
//     bit-by-bit tree walk, 4-byte bounded stream stores (FwdBitWriter) and plain bounded symbol stores.
// What a decoder reports for a damaged stream is the same in both forms: symbols are delivered one whole codeword at a
// time; a codeword that in_nbits cuts short is SCL_ST_TRUNCATED, a bit that leads to a missing child of an incomplete
// tree SCL_ST_STATE, bits left over after out_cap symbols SCL_ST_CAPACITY; d_consumed counts the whole codewords.
#include <string.h>

#include <vector>

#include "scl_ans_fast_io.h"
#include "scl_entry.h"
#include "scl_prefix_internal.h"

#define PF_THREADS 256
#define PF_RING_BYTES (32 * PF_THREADS * 4)

// ---- any-parameter kernels ---------------------------------------------------------------------------------------------
template <typename SYM>
__global__ void __launch_bounds__(256) prefix_encode_kernel(PrefixDev P, const SYM *__restrict__ sym, u64 sym_stride,
                                                           const u32 *__restrict__ lens, u32 chunk_len, u64 n_chunks,
                                                           u8 *__restrict__ out, u64 out_stride,
                                                           u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits,
                                                           u32 *__restrict__ status) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const u32 n = lens ? lens[c] : chunk_len;
    const SYM *src = sym + c * sym_stride;
    FwdBitWriter w;
    w.init(out + c * out_stride, out_stride);
    u32 st = 0;
    for (u32 i = 0; i < n; ++i) {
        u32 s = src[i];
        if (s >= P.K) {
            st |= SCL_ST_SYMBOL;
            s = 0;
        }
        const uint2 e = P.d_enc[s];
        w.put(e.x, e.y);
    }
    const u64 total = w.finish();
    if (w.overflow) st |= SCL_ST_CAPACITY;
    out_bit_off[c] = c * out_stride * 8;
    out_nbits[c] = (u32)total;
    if (status) status[c] = st;
}

template <typename SYM>
__global__ void __launch_bounds__(256) prefix_decode_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes,
                                                           const u64 *__restrict__ bit_off,
                                                           const u32 *__restrict__ in_nbits, u64 n_chunks,
                                                           SYM *__restrict__ out_sym, u64 out_stride, u32 out_cap,
                                                           u32 *__restrict__ out_lens, u32 *__restrict__ consumed,
                                                           u32 *__restrict__ status) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const u32 nb = in_nbits[c];
    BitReader r;
    r.init(in, in_size_bytes, bit_off[c], nb);
    SYM *dst = out_sym + c * out_stride;
    u32 pos = 0, count = 0, st = 0;
    while (pos < nb && st == 0) {
        if (count == out_cap) {
            st |= SCL_ST_CAPACITY;
            break;
        }
        const u32 avail = min(nb - pos, PF_MAX_LEN);
        const u32 bits = r.peek_at(r.pos + pos, avail) << (32u - avail);  // the next bits, left-aligned
        u32 node = 0;
        for (u32 d = 0;; ++d) {
            if (d == avail) {  // (a walk of 32 bits has ended in a leaf or a missing child: the tree is 32 deep)
                st |= SCL_ST_TRUNCATED;
                break;
            }
            const uint2 ch = P.d_nodes[node];
            const u32 next = ((bits >> (31u - d)) & 1u) ? ch.y : ch.x;
            if (next == PF_NONE) {
                st |= SCL_ST_STATE;
                break;
            }
            if (next & PF_LEAF) {
                dst[count++] = (SYM)(next & 0xFFFFu);
                pos += d + 1;
                break;
            }
            node = next;
        }
    }
    out_lens[c] = count;
    consumed[c] = pos;
    if (status) status[c] = st;
}

// ---- tuned kernels -----------------------------------------------------------------------------------------------------
typedef AnsFwdWriter<PF_THREADS, true> PfOut;
typedef AnsBitReader<PF_THREADS, false> PfIn;
#define PF_ENC_TAB PF_RING_BYTES           // uint2 {code, len} x 256
#define PF_LUT_BASE PF_RING_BYTES          // u16 x 2^T
#define PF_DEEP_BASE (PF_LUT_BASE + 4096)  // u32 x PF_DEEP_NODES

__global__ void __launch_bounds__(PF_THREADS, 4)
    prefix_encode_fast_kernel(PrefixDev P, const u8 *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens,
                              u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride,
                              u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[PF_ENC_TAB + 2048];
    const u32 tid = threadIdx.x;
    *reinterpret_cast<uint2 *>(lds + PF_ENC_TAB + tid * 8) = tid < P.K ? P.d_enc[tid] : make_uint2(0u, 0u);
    __syncthreads();
    const u64 chunk = (u64)blockIdx.x * PF_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 n = lens ? lens[chunk] : chunk_len;
    const u8 *src = sym + chunk * sym_stride;
    PfOut wr;
    wr.init(tid, out + chunk * out_stride, out_stride);
    u32 bad = 0;

    auto code_word = [&](u32 w, u32 cnt) {  // up to four symbols, first symbol in the low byte
#pragma unroll 1
        for (u32 j = 0; j < cnt; ++j) {
            u32 s = w & 0xFFu;
            w >>= 8;
            bad = max(bad, s);
            s = (s < P.K) ? s : 0u;
            const uint2 e = *reinterpret_cast<const uint2 *>(lds + PF_ENC_TAB + s * 8);
            wr.put_field(lds, e.x, e.y);
        }
        wr.maybe_flush(lds);  // <= 4 new words on top of <= 15 pending (ring of 32)
    };

    const u32 n_lines = n >> 7;
    const uint4 *src16 = reinterpret_cast<const uint4 *>(src);
    Line128 cur;
#pragma nounroll
    for (u32 t = 0; t < n_lines; ++t) {
        cur.load(src16 + 8 * t);
#pragma unroll 1
        for (u32 q = 0; q < 8; ++q) {
            const uint4 v = cur.v[0];
#pragma unroll
            for (int i = 0; i < 7; ++i) cur.v[i] = cur.v[i + 1];
            code_word(v.x, 4);
            code_word(v.y, 4);
            code_word(v.z, 4);
            code_word(v.w, 4);
        }
    }
    u32 i = n_lines << 7;
    for (; i + 4 <= n; i += 4) code_word(*reinterpret_cast<const u32 *>(src + i), 4);  // ragged tail
    if (i < n) {
        u32 w = 0;
        for (u32 j = 0; i + j < n; ++j) w |= (u32)src[i + j] << (8 * j);
        code_word(w, n - i);
    }
    const u64 total = wr.finish(lds);
    out_bit_off[chunk] = chunk * out_stride * 8;
    out_nbits[chunk] = (u32)total;
    if (status) status[chunk] = ((bad >= P.K) ? SCL_ST_SYMBOL : 0u) | (wr.overflow ? SCL_ST_CAPACITY : 0u);
}

__global__ void __launch_bounds__(PF_THREADS, 4)
    prefix_decode_fast_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                              const u32 *__restrict__ in_nbits, u64 n_chunks, u8 *__restrict__ out_sym, u64 out_stride,
                              u32 out_cap, u32 *__restrict__ out_lens, u32 *__restrict__ consumed,
                              u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[PF_DEEP_BASE + PF_DEEP_NODES * 4];
    const u32 tid = threadIdx.x;
    const u32 T = P.lut_bits;
    for (u32 i = tid; i < (1u << T); i += PF_THREADS) *reinterpret_cast<u16 *>(lds + PF_LUT_BASE + i * 2) = P.d_lut[i];
    for (u32 i = tid; i < P.n_deep; i += PF_THREADS) *reinterpret_cast<u32 *>(lds + PF_DEEP_BASE + i * 4) = P.d_deep[i];
    __syncthreads();
    const u64 chunk = (u64)blockIdx.x * PF_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 nb = in_nbits[chunk];
    PfIn rd;
    rd.init(in, in_size_bytes, bit_off[chunk], lds, tid);
    u8 *dst = out_sym + chunk * out_stride;
    const u32 lut_shift = 32u - T;
    u32 pos = 0, count = 0, st = 0;
    u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0, word = 0;  // the 16-byte piece that is filling, and its current word

    while (pos < nb && st == 0) {
        if (count == out_cap) {
            st |= SCL_ST_CAPACITY;
            break;
        }
        const u32 rem = nb - pos;
        const u32 e = *reinterpret_cast<const u16 *>(lds + PF_LUT_BASE + (rd.look() >> lut_shift) * 2);
        const u32 len = e & 15u, kind = (e >> 4) & 3u;
        u32 s = e >> 6;
        if (len > rem) {  // whatever lies behind the stream chose the entry: the codeword is cut short
            st |= SCL_ST_TRUNCATED;
            break;
        }
        if (kind == PF_KIND_SYM) {
            rd.advance(lds, len);
            pos += len;
        } else if (kind == PF_KIND_NONE) {
            st |= SCL_ST_STATE;
            break;
        } else {  // a code longer than T bits: on from deep node s, bit by bit
            rd.advance(lds, T);
            u32 node = s;
            for (u32 d = T;; ++d) {
                if (d == rem) {
                    st |= SCL_ST_TRUNCATED;
                    break;
                }
                const u32 bit = rd.look() >> 31;
                rd.advance(lds, 1);
                const u32 next = (*reinterpret_cast<const u32 *>(lds + PF_DEEP_BASE + node * 4) >> (16u * bit)) & 0xFFFFu;
                if (next == PF16_NONE) {
                    st |= SCL_ST_STATE;
                    break;
                }
                if (next & PF16_LEAF) {
                    s = next & 0xFFu;
                    pos += d + 1;
                    break;
                }
                node = next;
            }
            if (st) break;
        }
        word |= s << (8u * (count & 3u));
        if ((count & 3u) == 3u) {
            const u32 q = (count >> 2) & 3u;
            w0 = q == 0 ? word : w0;
            w1 = q == 1 ? word : w1;
            w2 = q == 2 ? word : w2;
            w3 = q == 3 ? word : w3;
            word = 0;
            if (q == 3) *reinterpret_cast<uint4 *>(dst + (count & ~15u)) = make_uint4(w0, w1, w2, w3);
            rd.maybe_refill(lds);  // four symbols: <= 4 words consumed since the last call
        }
        ++count;
    }
    // the last, partial piece: its whole words, then the bytes of the word that was filling
    {
        const u32 base = count & ~15u, full = (count & 15u) >> 2;
        u32 *d32 = reinterpret_cast<u32 *>(dst + base);
        if (full > 0) d32[0] = w0;
        if (full > 1) d32[1] = w1;
        if (full > 2) d32[2] = w2;
        for (u32 j = 0; j < (count & 3u); ++j) dst[base + 4 * full + j] = (u8)(word >> (8 * j));
    }
    out_lens[chunk] = count;
    consumed[chunk] = pos;
    if (status) status[chunk] = st;
}

// ---- host API ------------------------------------------------------------------------------------------------------------
extern "C" void scl_prefix_model_destroy(scl_prefix_model *m) {
    if (!m) return;
    if (m->d_enc) (void)hipFree(m->d_enc);
    if (m->d_nodes) (void)hipFree(m->d_nodes);
    if (m->d_lut) (void)hipFree(m->d_lut);
    if (m->d_deep) (void)hipFree(m->d_deep);
    delete m;
}

extern "C" int scl_prefix_model_create(const uint32_t *h_code, const uint8_t *h_len, uint32_t K, scl_prefix_model **out) {
    SCL_REQUIRE(out, "prefix_model_create: null output");
    *out = nullptr;
    SCL_REQUIRE(h_code && h_len && K >= 1 && K <= SCL_MAX_ALPHABET, "prefix_model_create: alphabet size %u outside 1..65536",
                K);
    // the code tree: children of node i (node 0 = root); a codeword that meets a leaf on its way, or ends on a node that
    // exists already, equals or is a prefix of another one (or the other way round)
    std::vector<uint2> nodes(1, make_uint2(PF_NONE, PF_NONE));
    std::vector<u32> depth(1, 0);
    u32 min_len = PF_MAX_LEN, max_len = 0, len_gcd = 0;
    for (u32 s = 0; s < K; ++s) {
        const u32 len = h_len[s];
        SCL_REQUIRE(len >= 1 && len <= PF_MAX_LEN, "prefix_model_create: symbol %u has a code of %u bits (1..32 are coded)", s,
                    len);
        const u32 code = len == 32 ? h_code[s] : (h_code[s] & ((1u << len) - 1u));  // the len low bits are the codeword
        min_len = len < min_len ? len : min_len;
        max_len = len > max_len ? len : max_len;
        for (u32 a = len, b = len_gcd; ; ) {  // gcd(len, len_gcd); gcd(len, 0) = len
            if (b == 0) {
                len_gcd = a;
                break;
            }
            const u32 t = a % b;
            a = b;
            b = t;
        }
        u32 node = 0;
        for (u32 d = 0; d < len; ++d) {
            const u32 bit = (code >> (len - 1 - d)) & 1u;
            u32 next = bit ? nodes[node].y : nodes[node].x;
            const bool last = d + 1 == len;
            SCL_REQUIRE(next == PF_NONE || (!(next & PF_LEAF) && !last),
                        "prefix_model_create: not prefix-free: the code of symbol %u equals, extends or is a prefix of another "
                        "symbol's", s);
            if (next == PF_NONE) {
                next = last ? (PF_LEAF | s) : (u32)nodes.size();
                (bit ? nodes[node].y : nodes[node].x) = next;
                if (!last) {
                    nodes.push_back(make_uint2(PF_NONE, PF_NONE));
                    depth.push_back(d + 1);
                }
            }
            node = next;
        }
    }
    const u32 T = max_len < PF_LUT_BITS ? max_len : PF_LUT_BITS;
    // tuned decoder: the internal nodes at depth >= T, numbered in the order they were made
    std::vector<u32> deep_of(nodes.size(), 0);
    u32 n_deep = 0;
    for (size_t i = 0; i < nodes.size(); ++i)
        if (depth[i] >= T) deep_of[i] = n_deep++;
    const bool fast = K <= 256 && n_deep <= PF_DEEP_NODES;
    std::vector<u16> lut;
    std::vector<u32> deep;
    if (fast) {
        lut.resize((size_t)1 << T);
        for (u32 i = 0; i < (1u << T); ++i) {
            u32 node = 0, entry = 0;
            for (u32 d = 0;; ++d) {
                if (d == T) {
                    entry = T | (PF_KIND_NODE << 4) | (deep_of[node] << 6);
                    break;
                }
                const u32 next = ((i >> (T - 1 - d)) & 1u) ? nodes[node].y : nodes[node].x;
                if (next == PF_NONE) {
                    entry = (d + 1) | (PF_KIND_NONE << 4);
                    break;
                }
                if (next & PF_LEAF) {
                    entry = (d + 1) | (PF_KIND_SYM << 4) | ((next & 0xFFu) << 6);
                    break;
                }
                node = next;
            }
            lut[i] = (u16)entry;
        }
        deep.assign(n_deep ? n_deep : 1, 0xFFFFFFFFu);
        auto child16 = [&](u32 ch) -> u32 {
            if (ch == PF_NONE) return PF16_NONE;
            return (ch & PF_LEAF) ? (PF16_LEAF | (ch & 0xFFu)) : deep_of[ch];
        };
        for (size_t i = 0; i < nodes.size(); ++i)
            if (depth[i] >= T) deep[deep_of[i]] = child16(nodes[i].x) | (child16(nodes[i].y) << 16);
    }
    std::vector<uint2> enc(K > 256 ? K : 256, make_uint2(0u, 0u));
    for (u32 s = 0; s < K; ++s) enc[s] = make_uint2(h_len[s] == 32 ? h_code[s] : (h_code[s] & ((1u << h_len[s]) - 1u)), h_len[s]);

    scl_prefix_model *m = new scl_prefix_model();
    m->device = scl_current_device();
    m->dev.K = K;
    m->dev.min_len = min_len;
    m->dev.max_len = max_len;
    m->dev.lut_bits = T;
    m->dev.len_gcd = len_gcd;
    m->dev.n_deep = fast ? n_deep : 0;
    m->fast = fast ? 1 : 0;
    const char *what = "prefix_model_create: device table upload";
    int rc = scl_upload(&m->d_enc, enc.data(), enc.size(), what);
    if (rc == SCL_OK) rc = scl_upload(&m->d_nodes, nodes.data(), nodes.size(), what);
    if (rc == SCL_OK && fast) rc = scl_upload(&m->d_lut, lut.data(), lut.size(), what);
    if (rc == SCL_OK && fast) rc = scl_upload(&m->d_deep, deep.data(), deep.size(), what);
    if (rc != SCL_OK) {
        scl_prefix_model_destroy(m);
        return rc;
    }
    m->dev.d_enc = m->d_enc;
    m->dev.d_nodes = m->d_nodes;
    m->dev.d_lut = m->d_lut;
    m->dev.d_deep = m->d_deep;
    *out = m;
    return SCL_OK;
}

// ---- the tuned kernel family of the byte entry points (scl_entry.h: SclFamily) -------------------------------------------
// The encoder checks its capacity (any slot will do); the tuned reader loads whole 16-byte blocks of the input.
static const SclFamily<scl_prefix_model> prefix_families[] = {
    {"prefix_fast", [](const scl_prefix_model *m, u64, bool tuned) { return tuned && m->fast; },
     scl_any_call<scl_prefix_model>,
     [](const scl_prefix_model *m, const SclDecodeArgs<u8> &a) { return scl_in_aligned(m, a) && a.in_size_bytes % 16 == 0; },
     scl_sym_rows_aligned<scl_prefix_model>, scl_out_rows_aligned<scl_prefix_model>,
     [](const scl_prefix_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, void *) -> int {
         scl_launch_encode(prefix_encode_fast_kernel, {(u32)((a.n_chunks + 255) / 256), 256}, st, m->dev, a);
         return SCL_OK;
     },
     [](const scl_prefix_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, void *) -> int {
         scl_launch_decode(prefix_decode_fast_kernel, {(u32)((a.n_chunks + 255) / 256), 256}, st, m->dev, a);
         return SCL_OK;
     },
     [](const scl_prefix_model *, u64, char *enc, char *dec, size_t cap) {
         scl_put_names(enc, dec, cap, "prefix_encode_fast_kernel", "prefix_decode_fast_kernel");
     }},
};

extern "C" int scl_prefix_model_info(const scl_prefix_model *m, scl_prefix_info *info) {
    SCL_REQUIRE(m && info, "prefix_model_info: null argument");
    info->K = m->dev.K;
    info->min_len = m->dev.min_len;
    info->max_len = m->dev.max_len;
    info->lut_bits = m->dev.lut_bits;
    info->fast_path = scl_first_served(prefix_families, m, 0, true) ? 1 : 0;  // the model's, whatever the thread's switch says
    info->device = m->device;
    return SCL_OK;
}

extern "C" int scl_prefix_kernel_names(const scl_prefix_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap) {
    return scl_kernel_names("prefix_kernel_names", prefix_families, m, n_chunks, enc, dec, cap, "prefix_encode_kernel",
                            "prefix_decode_kernel");
}

extern "C" uint64_t scl_prefix_slot_bytes(const scl_prefix_model *m, uint64_t n_symbols) {
    if (!m) return 0;
    // the writers store whole 32-bit words: up to three bytes behind the stream's last byte
    return scl_round_up((n_symbols * m->dev.max_len + 7) / 8 + 4, 128);
}

// ---- batch entry points: one body for uint8 symbols (the tuned kernels first) and uint16 symbols ------------------------
template <class SYM>
static int prefix_encode(const char *what, const scl_prefix_model *m, const SclEncodeArgs<SYM> &args, hipStream_t st) {
    return scl_encode_batch(what, prefix_families, m, args, st, nullptr, [&](const SclEncodeArgs<SYM> &a, const RowRelay &) -> int {
        scl_launch_encode(prefix_encode_kernel<SYM>, {(u32)((a.n_chunks + 255) / 256), 256}, st, m->dev, a);
        return SCL_OK;
    });
}

template <class SYM>
static int prefix_decode(const char *what, const scl_prefix_model *m, const SclDecodeArgs<SYM> &args, hipStream_t st) {
    return scl_decode_batch(what, prefix_families, m, args, st, nullptr, [&](const SclDecodeArgs<SYM> &a, const RowRelay &) -> int {
        scl_launch_decode(prefix_decode_kernel<SYM>, {(u32)((a.n_chunks + 255) / 256), 256}, st, m->dev, a);
        return SCL_OK;
    });
}

extern "C" int scl_prefix_encode_batch(const scl_prefix_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                                       const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks, uint8_t *d_out,
                                       uint64_t out_stride, uint64_t *d_out_bit_offset, uint32_t *d_out_nbits,
                                       uint32_t *d_status, void *stream) {
    const SclEncodeArgs<u8> a = {d_sym, sym_stride, d_lens, chunk_len, n_chunks,
                                 d_out, out_stride, d_out_bit_offset, d_out_nbits, d_status};
    return prefix_encode("prefix_encode_batch", m, a, (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_batch(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                       const uint64_t *d_bit_offset, const uint32_t *d_in_nbits, uint64_t n_chunks,
                                       uint8_t *d_out_sym, uint64_t out_stride, uint32_t out_cap, uint32_t *d_out_lens,
                                       uint32_t *d_consumed, uint32_t *d_status, void *stream) {
    const SclDecodeArgs<u8> a = {d_in, in_size_bytes, d_bit_offset, d_in_nbits, n_chunks, d_out_sym,
                                 out_stride, out_cap, d_out_lens, d_consumed, d_status};
    return prefix_decode("prefix_decode_batch", m, a, (hipStream_t)stream);
}

extern "C" int scl_prefix_encode_batch_u16(const scl_prefix_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                                           const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                           uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                           uint32_t *d_out_nbits, uint32_t *d_status, void *stream) {
    const SclEncodeArgs<u16> a = {d_sym, sym_stride, d_lens, chunk_len, n_chunks,
                                  d_out, out_stride, d_out_bit_offset, d_out_nbits, d_status};
    return prefix_encode("prefix_encode_batch_u16", m, a, (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_batch_u16(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                           const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                           uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                                           uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                           uint32_t *d_status, void *stream) {
    const SclDecodeArgs<u16> a = {d_in, in_size_bytes, d_bit_offset, d_in_nbits, n_chunks, d_out_sym,
                                  out_stride, out_cap, d_out_lens, d_consumed, d_status};
    return prefix_decode("prefix_decode_batch_u16", m, a, (hipStream_t)stream);
}

// ---- single-chunk host drivers -------------------------------------------------------------------------------------------
extern "C" int scl_prefix_encode_host(const scl_prefix_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                                      uint64_t out_cap_bytes, uint64_t *nbits) {
    return scl_host_encode_one(scl_host_encode_call<scl_prefix_encode_batch, scl_prefix_slot_bytes>(), m, h_sym, n, h_out,
                               out_cap_bytes, nbits);
}

extern "C" int scl_prefix_decode_host(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                      uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed) {
    return scl_host_decode_one(scl_host_decode_call<scl_prefix_decode_batch>(), m, h_in, in_nbits, h_out_sym, out_cap,
                               n_out, consumed);
}

extern "C" int scl_prefix_encode_host_u16(const scl_prefix_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                                          uint64_t out_cap_bytes, uint64_t *nbits) {
    return scl_host_encode_one(scl_host_encode_call<scl_prefix_encode_batch_u16, scl_prefix_slot_bytes>(), m,
                               (const u8 *)h_sym, n, h_out, out_cap_bytes, nbits);
}

extern "C" int scl_prefix_decode_host_u16(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                          uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed) {
    return scl_host_decode_one(scl_host_decode_call<scl_prefix_decode_batch_u16>(), m, h_in, in_nbits,
                               (u8 *)h_out_sym, out_cap, n_out, consumed);
}
