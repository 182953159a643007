// scl_uint.hip -- batched Golomb, universal and Elias-delta coding of uint32 values for gfx950, one wavefront lane per chunk.
//
// The lane-per-stream twin of scl_uint_block.hip (one block across the grid), built like scl_prefix.hip: the stream of a chunk
// is its codewords back to back, MSB first, front to back -- the reference's GolombUintEncoder(M) / UniversalUintEncoder /
// EliasDeltaUintEncoder -- nbits = the sum of the codeword lengths, 0 for an empty chunk, bit_offset[c] = 8 * c * out_stride.
// There is no table: the codeword is the rule of scl_uint_code.h, and a lane writes it as a run of ones and at most two
// fields of at most 32 bits, so EVERY uint32 value has a codeword here (the block kernels stop at 32 bits a codeword).
//
// Two forms, as for every coder:
//   any-parameter  FwdBitWriter / BitReader, plain bounded 4-byte stores: any alignment the argument checks allow.
//   tuned          256 lanes a workgroup, nothing in LDS but the 32 KiB word ring (four workgroups per CU): values in as
//                  128-byte lines (32 values), AnsFwdWriter<256, BOUNDED> out; AnsBitReader<256> in, decoded values out as
//                  whole 16-byte pieces, the last partial piece value by value.  Taken when value rows and output rows start on
//                  16-byte boundaries, d_in does and in_size_bytes is a multiple of 16; rows are never re-laid.
// Ring contracts under long codewords: the writer wants maybe_flush after at most 16 new words, the reader maybe_refill
// before it has consumed more than a few.  A Golomb run of hundreds of ones keeps neither by "four symbols, four words":
// the encoder puts runs with put_run (which flushes after every whole word), the decoder refills inside the run loop and
// between a codeword's two fields (SRC::relief of scl_uint_decode_wide).
// Statuses.  encode: SCL_ST_CAPACITY alone -- nbits is then the length needed (counted in 64 bits, saturating at 2^32 - 1),
// and a lane whose slot has overflowed stops emitting and only adds lengths.  decode: the verdicts of scl_uint_decode_wide
// (SCL_ST_TRUNCATED, SCL_ST_SIZE) and SCL_ST_CAPACITY for bits left after out_cap values; the whole codewords in front of a
// fault are delivered, d_consumed counts their bits.  DESIGN.md 3.5.3.
#include "scl_ans_fast_io.h"
#include "scl_uint_code.h"

#define UI_THREADS 256
#define UI_RING_BYTES (32 * UI_THREADS * 4)
#define UI_RUN_STEP 1024u  // ones put between two looks at the writer's overflow flag

// ---- what both forms share: a chunk's codewords into a writer, a stream's codewords out of a source ---------------------
// W: put(v, w <= 32), put_run(bit, count), full().  Returns the codeword's length.
template <class W>
__device__ __forceinline__ u64 ui_put(const SclUintRule &C, W &w, u32 x) {
    const SclUintFields f = scl_uint_fields(C, x);
    if (!w.full()) {
        u32 run = f.run;
        while (run && !w.full()) {  // (a run that no slot holds ends here, not after x / M ones)
            const u32 k = run < UI_RUN_STEP ? run : UI_RUN_STEP;
            w.put_run(1u, k);
            run -= k;
        }
        w.put(f.f0, f.n0);
        if (C.kind != SCL_UINT_GOLOMB) w.put(f.f1, f.n1);
    }
    return scl_uint_fields_len(f);
}

__device__ __forceinline__ void ui_encode_done(u64 total, u64 chunk, u64 out_stride, u64 *__restrict__ out_bit_off,
                                               u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    out_bit_off[chunk] = chunk * out_stride * 8;
    out_nbits[chunk] = total < 0xFFFFFFFFull ? (u32)total : 0xFFFFFFFFu;
    // the writers store whole words: the stream fits iff its last word does
    if (status) status[chunk] = ((total + 31) / 32 * 4 > out_stride) ? SCL_ST_CAPACITY : 0u;
}

// ---- any-parameter kernels ---------------------------------------------------------------------------------------------
struct UiPlainOut : FwdBitWriter {  // (FwdBitWriter::put takes a field of 0 bits as it is)
    __device__ __forceinline__ bool full() const { return overflow != 0; }
};

struct UiPlainIn {
    BitReader r;
    __device__ __forceinline__ u32 look() const { return r.peek_at(r.pos, 32); }  // zeros behind the stream
    __device__ __forceinline__ void skip(u32 n) { r.pos += n; }
    __device__ __forceinline__ void relief() {}
};

__global__ void __launch_bounds__(256)
    uint_encode_kernel(SclUintRule C, const u32 *__restrict__ val, u64 val_stride, const u32 *__restrict__ lens, u32 chunk_len,
                       u64 n_chunks, u8 *__restrict__ out, u64 out_stride, u64 *__restrict__ out_bit_off,
                       u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const u32 n = lens ? lens[c] : chunk_len;
    const u32 *src = val + c * val_stride;
    UiPlainOut w;
    w.init(out + c * out_stride, out_stride);
    u64 total = 0;
    for (u32 i = 0; i < n; ++i) total += ui_put(C, w, src[i]);
    if (!w.full()) (void)w.finish();
    ui_encode_done(total, c, out_stride, out_bit_off, out_nbits, status);
}

__global__ void __launch_bounds__(256)
    uint_decode_kernel(SclUintRule C, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                       const u32 *__restrict__ in_nbits, u64 n_chunks, u32 *__restrict__ out_val, u64 out_stride, u32 out_cap,
                       u32 *__restrict__ out_lens, u32 *__restrict__ consumed, u32 *__restrict__ status) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const u32 nb = in_nbits[c];
    UiPlainIn s;
    s.r.init(in, in_size_bytes, bit_off[c], nb);
    u32 *dst = out_val + c * out_stride;
    u32 pos = 0, count = 0, st = 0;
    while (pos < nb) {
        if (count == out_cap) {
            st = SCL_ST_CAPACITY;
            break;
        }
        u32 len = 0, x = 0;
        st = scl_uint_decode_wide(C, s, nb - pos, len, x);
        if (st) break;
        dst[count++] = x;
        pos += len;
    }
    out_lens[c] = count;
    consumed[c] = pos;
    if (status) status[c] = st;
}

// ---- tuned kernels -----------------------------------------------------------------------------------------------------
struct UiRingOut {
    AnsFwdWriter<UI_THREADS, true> wr;
    char *lds;
    __device__ __forceinline__ bool full() const { return wr.overflow != 0; }
    __device__ __forceinline__ void put(u32 v, u32 w) { wr.put_field(lds, v, w); }
    __device__ __forceinline__ void put_run(u32 bit, u32 count) { wr.put_run(lds, bit, count); }
};

struct UiRingIn {
    AnsBitReader<UI_THREADS, false> rd;
    char *lds;
    __device__ __forceinline__ u32 look() const { return rd.look(); }
    __device__ __forceinline__ void skip(u32 n) { rd.advance(lds, n); }
    __device__ __forceinline__ void relief() { rd.maybe_refill(lds); }
};

__global__ void __launch_bounds__(UI_THREADS, 4)
    uint_encode_fast_kernel(SclUintRule C, const u32 *__restrict__ val, u64 val_stride, const u32 *__restrict__ lens,
                            u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride, u64 *__restrict__ out_bit_off,
                            u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[UI_RING_BYTES];
    const u32 tid = threadIdx.x;
    const u64 chunk = (u64)blockIdx.x * UI_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 n = lens ? lens[chunk] : chunk_len;
    const u32 *src = val + chunk * val_stride;
    UiRingOut w;
    w.lds = lds;
    w.wr.init(tid, out + chunk * out_stride, out_stride);
    u64 total = 0;

    auto code4 = [&](const uint4 &v) {  // a run leaves fewer than 32 bits pending: <= 2 new words a value, <= 9 here
        total += ui_put(C, w, v.x);
        total += ui_put(C, w, v.y);
        total += ui_put(C, w, v.z);
        total += ui_put(C, w, v.w);
        w.wr.maybe_flush(lds);
    };

    const u32 n_lines = n >> 5;
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
            code4(v);
        }
    }
    u32 i = n_lines << 5;
    for (; i + 4 <= n; i += 4) code4(*reinterpret_cast<const uint4 *>(src + i));  // ragged tail
    for (; i < n; ++i) total += ui_put(C, w, src[i]);                               // <= 3 values: <= 7 new words
    (void)w.wr.finish(lds);
    ui_encode_done(total, chunk, out_stride, out_bit_off, out_nbits, status);
}

__global__ void __launch_bounds__(UI_THREADS, 4)
    uint_decode_fast_kernel(SclUintRule C, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                            const u32 *__restrict__ in_nbits, u64 n_chunks, u32 *__restrict__ out_val, u64 out_stride,
                            u32 out_cap, u32 *__restrict__ out_lens, u32 *__restrict__ consumed, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[UI_RING_BYTES];
    const u32 tid = threadIdx.x;
    const u64 chunk = (u64)blockIdx.x * UI_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 nb = in_nbits[chunk];
    UiRingIn s;
    s.lds = lds;
    s.rd.init(in, in_size_bytes, bit_off[chunk], lds, tid);
    u32 *dst = out_val + chunk * out_stride;
    u32 pos = 0, count = 0, st = 0;
    u32 w0 = 0, w1 = 0, w2 = 0;  // the 16-byte piece that is filling

    // every codeword passes a relief of the rule: at most two words are consumed between two refills
    while (pos < nb) {
        if (count == out_cap) {
            st = SCL_ST_CAPACITY;
            break;
        }
        u32 len = 0, x = 0;
        st = scl_uint_decode_wide(C, s, nb - pos, len, x);
        if (st) break;
        pos += len;
        const u32 q = count & 3u;
        w0 = q == 0 ? x : w0;
        w1 = q == 1 ? x : w1;
        w2 = q == 2 ? x : w2;
        if (q == 3) *reinterpret_cast<uint4 *>(dst + (count & ~3u)) = make_uint4(w0, w1, w2, x);
        ++count;
    }
    {  // the last, partial piece
        const u32 base = count & ~3u, left = count & 3u;
        if (left > 0) dst[base] = w0;
        if (left > 1) dst[base + 1] = w1;
        if (left > 2) dst[base + 2] = w2;
    }
    out_lens[chunk] = count;
    consumed[chunk] = pos;
    if (status) status[chunk] = st;
}

// ---- host API ------------------------------------------------------------------------------------------------------------
// the tuned pair runs when the rows allow it and the calling thread has not asked for the any-parameter kernels
static bool ui_rows16(const void *p, u64 stride_elems) { return (((uintptr_t)p | (stride_elems * 4)) & 15) == 0; }
static bool ui_enc_tuned(const SclEncodeArgs<u32> &a) { return !scl_force_generic() && ui_rows16(a.d_sym, a.sym_stride); }
static bool ui_dec_tuned(const SclDecodeArgs<u32> &a) {
    return !scl_force_generic() && ui_rows16(a.d_out_sym, a.out_stride) && ((uintptr_t)a.d_in & 15) == 0 &&
           a.in_size_bytes % 16 == 0;
}

extern "C" uint64_t scl_uint_slot_bytes(const scl_uint_code *code, uint64_t n_values, uint32_t max_value) {
    if (!code || code->kind > SCL_UINT_ELIAS_DELTA) return 0;
    if (code->kind == SCL_UINT_GOLOMB && (code->M < 1 || code->M >= (1u << 31))) return 0;
    // no codeword of a value up to max_value is longer than max_value's: the length of all three codes never decreases in x
    const u64 len = scl_uint_fields_len(scl_uint_fields(scl_uint_rule_make(code->kind, code->M), max_value));
    const unsigned __int128 bits = (unsigned __int128)n_values * len;
    if (bits >> 62) return 0;
    // the writers store whole 32-bit words: up to three bytes behind the stream's last byte
    return scl_round_up(((u64)bits + 7) / 8 + 4, 128);
}

extern "C" int scl_uint_encode_batch(const scl_uint_code *code, const uint32_t *d_val, uint64_t val_stride,
                                     const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks, uint8_t *d_out,
                                     uint64_t out_stride, uint64_t *d_out_bit_offset, uint32_t *d_out_nbits,
                                     uint32_t *d_status, void *stream) {
    const char *what = "uint_encode_batch";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    const SclEncodeArgs<u32> a = {d_val, val_stride, d_lens, chunk_len, n_chunks,
                                  d_out, out_stride, d_out_bit_offset, d_out_nbits, d_status};
    SCL_REQUIRE(a.d_sym && a.d_out && a.d_bit_off && a.d_nbits, "%s: null pointer argument", what);
    SCL_REQUIRE(a.out_stride % 16 == 0 && a.out_stride > 0 && a.out_stride * 8 < (1ull << 32), "%s: bad out_stride %llu", what,
                (unsigned long long)a.out_stride);
    SCL_REQUIRE(((uintptr_t)a.d_out & 15) == 0 && ((uintptr_t)a.d_sym & 3) == 0,
                "%s: d_out must be 16-byte aligned, d_val 4-byte aligned", what);
    if (n_chunks == 0) return SCL_OK;
    const hipStream_t st = (hipStream_t)stream;
    const SclGrid grid = {(u32)((n_chunks + 255) / 256), 256};
    if (ui_enc_tuned(a))
        scl_launch_encode(uint_encode_fast_kernel, grid, st, C, a);
    else
        scl_launch_encode(uint_encode_kernel, grid, st, C, a);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_uint_decode_batch(const scl_uint_code *code, const uint8_t *d_in, uint64_t in_size_bytes,
                                     const uint64_t *d_bit_offset, const uint32_t *d_in_nbits, uint64_t n_chunks,
                                     uint32_t *d_out_val, uint64_t out_stride, uint32_t out_cap, uint32_t *d_out_lens,
                                     uint32_t *d_consumed, uint32_t *d_status, void *stream) {
    const char *what = "uint_decode_batch";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    const SclDecodeArgs<u32> a = {d_in, in_size_bytes, d_bit_offset, d_in_nbits, n_chunks, d_out_val,
                                  out_stride, out_cap, d_out_lens, d_consumed, d_status};
    SCL_REQUIRE(a.d_in && a.d_bit_off && a.d_in_nbits && a.d_out_sym && a.d_out_lens && a.d_consumed,
                "%s: null pointer argument", what);
    SCL_REQUIRE(((uintptr_t)a.d_in & 3) == 0 && ((uintptr_t)a.d_out_sym & 3) == 0,
                "%s: d_in and d_out_val must be 4-byte aligned", what);
    if (n_chunks == 0) return SCL_OK;
    const hipStream_t st = (hipStream_t)stream;
    const SclGrid grid = {(u32)((n_chunks + 255) / 256), 256};
    if (ui_dec_tuned(a))
        scl_launch_decode(uint_decode_fast_kernel, grid, st, C, a);
    else
        scl_launch_decode(uint_decode_kernel, grid, st, C, a);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

// the two kernels of a batch of aligned rows, as rocprofv3 prints them
extern "C" int scl_uint_kernel_names(const scl_uint_code *code, uint64_t n_chunks, char *enc, char *dec, uint64_t cap) {
    const char *what = "uint_kernel_names";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE((enc || dec) && cap >= 96, "%s: null argument or a buffer below 96 bytes", what);
    (void)n_chunks;
    const bool tuned = !scl_force_generic();
    if (enc) snprintf(enc, (size_t)cap, "%s", tuned ? "uint_encode_fast_kernel" : "uint_encode_kernel");
    if (dec) snprintf(dec, (size_t)cap, "%s", tuned ? "uint_decode_fast_kernel" : "uint_decode_kernel");
    return SCL_OK;
}

// ---- the rule on the host, for tests -------------------------------------------------------------------------------------
extern "C" int scl_uint_fields_host(const scl_uint_code *code, uint32_t x, uint32_t *run, uint32_t *fields, uint32_t *widths) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked("uint_fields_host", code, &C)) return rc;
    SCL_REQUIRE(run && fields && widths, "uint_fields_host: null pointer argument");
    const SclUintFields f = scl_uint_fields(C, x);
    *run = f.run;
    fields[0] = f.f0, fields[1] = f.f1;
    widths[0] = f.n0, widths[1] = f.n1;
    return SCL_OK;
}

struct UiHostIn {  // bits from a byte buffer, zeros behind it
    const u8 *buf;
    u64 size, pos;
    u32 look() const {
        u64 v = 0;
        for (u64 i = 0; i < 5; ++i) v = (v << 8) | (pos / 8 + i < size ? buf[pos / 8 + i] : 0u);
        return (u32)(v >> (8 - pos % 8));
    }
    void skip(u32 n) { pos += n; }
    void relief() {}
};

extern "C" int scl_uint_decode_wide_one_host(const scl_uint_code *code, const uint8_t *buf, uint64_t buf_bytes,
                                             uint64_t bit_pos, uint32_t rem, uint32_t *len, uint32_t *x) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked("uint_decode_wide_one_host", code, &C)) return rc;
    SCL_REQUIRE(buf && len && x, "uint_decode_wide_one_host: null pointer argument");
    SCL_REQUIRE(rem >= 1, "uint_decode_wide_one_host: rem = 0: at least one bit belongs to the stream");
    *len = *x = 0;
    UiHostIn s = {buf, buf_bytes, bit_pos};
    return (int)scl_uint_decode_wide(C, s, rem, *len, *x);
}
