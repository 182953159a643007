// scl_entry.h -- what every coder's C entry points share: the argument checks of the batch calls, the walk over a coder's
// table of tuned kernel families that chooses the kernels (and names them), the prologue of the wave-striped calls and
// the single-chunk host drivers.  Host code only; included by scl_{rans,tans,range,prefix,aec}.hip.
#pragma once

#include <type_traits>

#include "scl_common.h"

// ---- argument checks of the batch entry points -----------------------------------------------------------------------
// Run first, in this order: null pointers, the byte path's alphabet (K <= 256; wider ones take the *_u16 twin), the
// model's device (scl_check_device), then
//   encode: out_stride a positive multiple of 16; on linear slots also below 512 MiB (32-bit bit counts), d_out 16-byte
//           and uint16 symbol rows 2-byte aligned;
//   decode: on linear slots d_in 4-byte and uint16 output rows 2-byte aligned.
// Striped slots check the rest in scl_striped_encode / scl_striped_decode.  MODEL is any coder's handle (dev.K, device).
enum SclRows { SCL_ROWS_U8, SCL_ROWS_U16, SCL_ROWS_STRIPED };
template <class SYM>
constexpr SclRows scl_rows_of() { return sizeof(SYM) == 1 ? SCL_ROWS_U8 : SCL_ROWS_U16; }

template <class MODEL, class SYM>
int scl_check_encode(const char *what, SclRows rows, const MODEL *m, const SclEncodeArgs<SYM> &a) {
    SCL_REQUIRE(m && a.d_sym && a.d_out && a.d_bit_off && a.d_nbits, "%s: null pointer argument", what);
    SCL_REQUIRE(rows != SCL_ROWS_U8 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K,
                what);
    if (int rc = scl_check_device(m->device, what)) return rc;
    SCL_REQUIRE(a.out_stride % 16 == 0 && a.out_stride > 0 &&
                    (rows == SCL_ROWS_STRIPED || a.out_stride * 8 < (1ull << 32)),
                "%s: bad out_stride %llu", what, (unsigned long long)a.out_stride);
    if (rows == SCL_ROWS_STRIPED) return SCL_OK;
    SCL_REQUIRE(((uintptr_t)a.d_out & 15) == 0 && (rows == SCL_ROWS_U8 || ((uintptr_t)a.d_sym & 1) == 0),
                "%s: d_out must be 16-byte aligned%s", what, rows == SCL_ROWS_U8 ? "" : ", d_sym 2-byte aligned");
    return SCL_OK;
}

template <class MODEL, class SYM>
int scl_check_decode(const char *what, SclRows rows, const MODEL *m, const SclDecodeArgs<SYM> &a) {
    SCL_REQUIRE(m && a.d_in && a.d_bit_off && a.d_in_nbits && a.d_out_sym && a.d_out_lens && a.d_consumed,
                "%s: null pointer argument", what);
    SCL_REQUIRE(rows != SCL_ROWS_U8 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K,
                what);
    if (int rc = scl_check_device(m->device, what)) return rc;
    if (rows == SCL_ROWS_STRIPED) return SCL_OK;
    SCL_REQUIRE(((uintptr_t)a.d_in & 3) == 0 && (rows == SCL_ROWS_U8 || ((uintptr_t)a.d_out_sym & 1) == 0),
                "%s: d_in must be 4-byte aligned%s", what, rows == SCL_ROWS_U8 ? "" : ", d_out_sym 2-byte aligned");
    return SCL_OK;
}

// ---- kernel choice of the batch entry points ---------------------------------------------------------------------------
// A coder lists its tuned kernel families in priority order; the batch calls (scl_encode_batch / scl_decode_batch below)
// and the calls that only report the choice (scl_first_served, scl_kernel_names) read the same list.  MODEL: the coder's
// handle.  Byte symbols only: uint16 symbols run the coder's any-parameter kernels.
template <class MODEL>
struct SclFamily {
    const char *name;  // for comments and error text
    // Does the family serve the model?  max_symbols: the longest chunk (chunk_len / out_cap).  tuned: the calling thread
    // lets the tuned kernels run (!scl_force_generic(); the calls that report the MODEL pass true).  Environment switches
    // that move a model from one family to another are read in here.
    bool (*served)(const MODEL *m, u64 max_symbols, bool tuned);
    // what the kernels need of the call that re-laying its rows cannot give ...
    bool (*enc_call_ok)(const MODEL *m, const SclEncodeArgs<u8> &a);
    bool (*dec_call_ok)(const MODEL *m, const SclDecodeArgs<u8> &a);
    // ... and of the rows, once the relay has run
    bool (*enc_rows_ok)(const MODEL *m, const SclEncodeArgs<u8> &a);
    bool (*dec_rows_ok)(const MODEL *m, const SclDecodeArgs<u8> &a);
    // start the kernels; `call`: what the coder's entry point handed to the walk (the arithmetic coder's scratch)
    int (*encode)(const MODEL *m, const SclEncodeArgs<u8> &a, hipStream_t st, void *call);
    int (*decode)(const MODEL *m, const SclDecodeArgs<u8> &a, hipStream_t st, void *call);
    // the two kernels of a batch of n_chunks aligned, equally long rows, as rocprofv3 prints them (null: the coder has no
    // *_kernel_names call)
    void (*names)(const MODEL *m, u64 n_chunks, char *enc, char *dec, size_t cap);
};

// predicates most families share
template <class MODEL>
bool scl_any_call(const MODEL *, const SclEncodeArgs<u8> &) { return true; }
template <class MODEL>
bool scl_in_aligned(const MODEL *, const SclDecodeArgs<u8> &a) { return ((uintptr_t)a.d_in & 15) == 0; }
template <class MODEL>
bool scl_sym_rows_aligned(const MODEL *, const SclEncodeArgs<u8> &a) { return scl_rows_aligned(a.d_sym, a.sym_stride); }
template <class MODEL>
bool scl_out_rows_aligned(const MODEL *, const SclDecodeArgs<u8> &a) { return scl_rows_aligned(a.d_out_sym, a.out_stride); }

static inline void scl_put_names(char *enc, char *dec, size_t cap, const char *enc_name, const char *dec_name) {
    if (enc) snprintf(enc, cap, "%s", enc_name);
    if (dec) snprintf(dec, cap, "%s", dec_name);
}

// the family that runs a batch of aligned rows in slots of the coder's size: the first that serves the model, or null
template <class MODEL, size_t N>
const SclFamily<MODEL> *scl_first_served(const SclFamily<MODEL> (&families)[N], const MODEL *m, u64 max_symbols, bool tuned) {
    for (const SclFamily<MODEL> &f : families)
        if (f.served(m, max_symbols, tuned)) return &f;
    return nullptr;
}

// the body of a *_kernel_names call (any_enc / any_dec: the coder's any-parameter kernels)
template <class MODEL, size_t N>
int scl_kernel_names(const char *what, const SclFamily<MODEL> (&families)[N], const MODEL *m, u64 n_chunks, char *enc,
                     char *dec, u64 cap, const char *any_enc, const char *any_dec) {
    SCL_REQUIRE(m && (enc || dec) && cap >= 96, "%s: null argument or a buffer below 96 bytes", what);
    if (const SclFamily<MODEL> *f = scl_first_served(families, m, 0, !scl_force_generic()))
        f->names(m, n_chunks, enc, dec, (size_t)cap);
    else
        scl_put_names(enc, dec, (size_t)cap, any_enc, any_dec);
    return SCL_OK;
}

// The body of every *_encode_batch / *_decode_batch call on linear slots: the argument checks, nothing to do for an empty
// batch, then the FIRST family that serves the model and can take the call runs it.  Rows that do not start on 16-byte
// boundaries are re-laid first (RowRelay) if and only if some family that serves the model could then take them; a
// decoder's rows are copied back at the end.  any(a, relay) starts the coder's any-parameter kernels on the arguments as
// the walk leaves them (relay.failed: rows had to be re-laid and the scratch could not be had) when no family took the
// call, and for uint16 symbols.
template <class MODEL, size_t N, class SYM, class ANY>
int scl_encode_batch(const char *what, const SclFamily<MODEL> (&families)[N], const MODEL *m, const SclEncodeArgs<SYM> &args,
                     hipStream_t st, void *call, ANY any) {
    static_assert(N <= 32, "one bit per family");
    if (int rc = scl_check_encode(what, scl_rows_of<SYM>(), m, args)) return rc;
    if (args.n_chunks == 0) return SCL_OK;
    SclEncodeArgs<SYM> a = args;
    RowRelay relay;
    if constexpr (sizeof(SYM) == 1) {
        const bool tuned = !scl_force_generic();
        u32 takes = 0;  // bit i: family i serves the model and the call has what it needs
        for (size_t i = 0; i < N; ++i)
            if (families[i].served(m, a.chunk_len, tuned) && families[i].enc_call_ok(m, a)) takes |= 1u << i;
        if (takes)
            if (int rc = relay.in(a, st)) return rc;
        for (size_t i = 0; i < N; ++i) {
            if (!(takes >> i & 1) || !families[i].enc_rows_ok(m, a)) continue;
            if (int rc = families[i].encode(m, a, st, call)) return rc;
            SCL_HIP_TRY(hipGetLastError());
            return SCL_OK;
        }
    }
    if (int rc = any(a, relay)) return rc;
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class MODEL, size_t N, class SYM, class ANY>
int scl_decode_batch(const char *what, const SclFamily<MODEL> (&families)[N], const MODEL *m, const SclDecodeArgs<SYM> &args,
                     hipStream_t st, void *call, ANY any) {
    static_assert(N <= 32, "one bit per family");
    if (int rc = scl_check_decode(what, scl_rows_of<SYM>(), m, args)) return rc;
    if (args.n_chunks == 0) return SCL_OK;
    SclDecodeArgs<SYM> a = args;
    RowRelay relay;
    if constexpr (sizeof(SYM) == 1) {
        const bool tuned = !scl_force_generic();
        u32 takes = 0;
        for (size_t i = 0; i < N; ++i)
            if (families[i].served(m, a.out_cap, tuned) && families[i].dec_call_ok(m, a)) takes |= 1u << i;
        if (takes)
            if (int rc = relay.out_begin(a, st)) return rc;
        for (size_t i = 0; i < N; ++i) {
            if (!(takes >> i & 1) || !families[i].dec_rows_ok(m, a)) continue;
            if (int rc = families[i].decode(m, a, st, call)) return rc;
            SCL_HIP_TRY(hipGetLastError());
            return relay.out_end(a);
        }
    }
    if (int rc = any(a, relay)) return rc;
    SCL_HIP_TRY(hipGetLastError());
    return relay.out_end(a);
}

// The slot of the rANS and tANS coders (scl_rans_slot_bytes / scl_tans_slot_bytes): header, final state and the worst case
// of every symbol, whole bytes plus the word the writers store past the stream's end, in lines of 128 bytes.
template <class MODEL>
u64 scl_ans_slot_bytes(const MODEL *m, u64 n_symbols) {
    if (!m) return 0;
    const u64 bits = (u64)m->dev.size_bits + m->dev.nsb + n_symbols * (u64)m->max_bits_per_symbol;
    return scl_round_up((bits + 7) / 8 + 4, 128);
}

// ---- wave-striped slots (ABI version 8): the body of every *_batch_striped call, after its argument checks ------------
// Only the tuned kernels have a striped form: a model they do not serve (`served` = scl_*_striped_ok) is refused, and so
// is a call made while the calling thread keeps them out (scl_set_any_parameter_kernels).  Slots start on 16-byte
// boundaries and stay below 2^24 bytes (32-bit offsets per workgroup); an encoder's are at least min_slot bytes (0: no
// bound -- the range coder reports a short slot as SCL_ST_CAPACITY).  Rows that do not start on 16-byte boundaries go
// through the row relay; launch(a) then starts the coder's striped kernel on the arguments it is given (the caller's,
// with the rows re-laid where they had to be; a decoder's in_size_bytes is the slot stride).
template <class LAUNCH>
int scl_striped_encode(const char *what, bool served, u64 min_slot, SclEncodeArgs<u8> a, hipStream_t st, LAUNCH launch) {
    SCL_REQUIRE(served, "%s: this model is not served by the striped kernels (see scl_*_striped_ok)", what);
    SCL_REQUIRE(!scl_force_generic(), "%s: the calling thread keeps the tuned kernels out; striped slots have no other", what);
    SCL_REQUIRE(((uintptr_t)a.d_out & 15) == 0, "%s: d_out must be 16-byte aligned", what);
    SCL_REQUIRE(a.out_stride >= min_slot && a.out_stride < (1ull << 24),
                "%s: out_stride %llu: striped slots need scl_*_slot_bytes(chunk_len) <= out_stride < 2^24", what,
                (unsigned long long)a.out_stride);
    if (a.n_chunks == 0) return SCL_OK;
    RowRelay relay;
    if (int rc = relay.in(a, st)) return rc;
    if (!scl_rows_aligned(a.d_sym, a.sym_stride)) {
        scl_set_error("%s: out of device memory re-laying unaligned symbol rows (hipMallocAsync failed)", what);
        return SCL_E_ALLOC;
    }
    launch(a);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class LAUNCH>
int scl_striped_decode(const char *what, bool served, SclDecodeArgs<u8> a, hipStream_t st, LAUNCH launch) {
    SCL_REQUIRE(served, "%s: this model is not served by the striped kernels (see scl_*_striped_ok)", what);
    SCL_REQUIRE(!scl_force_generic(), "%s: the calling thread keeps the tuned kernels out; striped slots have no other", what);
    SCL_REQUIRE(((uintptr_t)a.d_in & 15) == 0 && a.in_size_bytes % 16 == 0 && a.in_size_bytes > 0 &&
                    a.in_size_bytes < (1ull << 24),
                "%s: d_in must be 16-byte aligned and in_stride a multiple of 16 below 2^24", what);
    if (a.n_chunks == 0) return SCL_OK;
    RowRelay relay;  // output rows the kernels cannot store to go through aligned scratch and are copied back
    if (int rc = relay.out_begin(a, st)) return rc;
    if (!scl_rows_aligned(a.d_out_sym, a.out_stride)) {
        scl_set_error("%s: out of device memory re-laying unaligned output rows (hipMallocAsync failed)", what);
        return SCL_E_ALLOC;
    }
    launch(a);
    SCL_HIP_TRY(hipGetLastError());
    return relay.out_end(a);
}

// ---- single-chunk host drivers over a batch entry point ----------------------------------------------------------------
// SclBatch<decltype(BATCH)> reads a batch entry point's model and symbol types off its signature, and how many arguments
// follow d_status: the stream alone, (d_scratch, scratch_bytes, stream), or (d_state, state_bytes, n_coders, stream).
template <class F>
struct SclBatch;
template <class M, class S, class... TAIL>  // *_encode_batch*
struct SclBatch<int (*)(const M *, const S *, u64, const u32 *, u32, u64, u8 *, u64, u64 *, u32 *, u32 *, TAIL...)> {
    using Model = M;
    using Sym = S;
    static constexpr size_t tail = sizeof...(TAIL);
};
template <class M, class S, class... TAIL>  // *_decode_batch*
struct SclBatch<int (*)(const M *, const u8 *, u64, const u64 *, const u32 *, u64, S *, u64, u32, u32 *, u32 *, u32 *,
                        TAIL...)> {
    using Model = M;
    using Sym = S;
    static constexpr size_t tail = sizeof...(TAIL);
};

// one chunk on the default stream; the host driver's device scratch is the coder's scratch, or its state (one coder)
template <auto BATCH, class... A>
int scl_batch_one(void *d_scratch, u64 scratch_bytes, A... args) {
    constexpr size_t tail = SclBatch<decltype(BATCH)>::tail;
    if constexpr (tail == 1) return BATCH(args..., nullptr);
    else if constexpr (tail == 3) return BATCH(args..., d_scratch, scratch_bytes, nullptr);
    else return BATCH(args..., d_scratch, scratch_bytes, 1, nullptr);
}

// ROW_STRIDE(model, n): the symbol row's stride when it is not n (a row's stride is free)
template <auto BATCH, auto ROW_STRIDE>
int scl_host_run_enc(const void *model, const SclEncodeArgs<u8> &a, void *d_scratch, u64 scratch_bytes) {
    using B = SclBatch<decltype(BATCH)>;
    const auto *m = (const typename B::Model *)model;
    u64 sym_stride = a.sym_stride;
    if constexpr (!std::is_null_pointer_v<decltype(ROW_STRIDE)>) sym_stride = ROW_STRIDE(m, a.chunk_len);
    return scl_batch_one<BATCH>(d_scratch, scratch_bytes, m, (const typename B::Sym *)a.d_sym, sym_stride, a.d_lens,
                                a.chunk_len, a.n_chunks, a.d_out, a.out_stride, a.d_bit_off, a.d_nbits, a.d_status);
}

// decoded rows: byte rows padded to a multiple of 16 (what the tuned decoders store), uint16 rows as they are
template <auto BATCH>
int scl_host_run_dec(const void *model, const SclDecodeArgs<u8> &a, void *d_scratch, u64 scratch_bytes) {
    using B = SclBatch<decltype(BATCH)>;
    using S = typename B::Sym;
    const u64 out_stride = sizeof(S) == 1 ? scl_round_up((u64)a.out_cap + 1, 16) : (u64)a.out_cap + 1;
    return scl_batch_one<BATCH>(d_scratch, scratch_bytes, (const typename B::Model *)model, a.d_in, a.in_size_bytes,
                                a.d_bit_off, a.d_in_nbits, a.n_chunks, (S *)a.d_out_sym, out_stride, a.out_cap,
                                a.d_out_lens, a.d_consumed, a.d_status);
}

// SLOT / SCRATCH: the coder's scl_*_slot_bytes(model, n) / scratch size (model, 1 chunk), nullptr if it needs none
template <auto BATCH, auto SLOT, auto SCRATCH = nullptr, auto ROW_STRIDE = nullptr>
HostEncodeCall scl_host_encode_call() {
    using B = SclBatch<decltype(BATCH)>;
    HostEncodeCall c = {scl_host_run_enc<BATCH, ROW_STRIDE>,
                        [](const void *m, u64 n) -> u64 { return SLOT((const typename B::Model *)m, n); }, nullptr};
    if constexpr (!std::is_null_pointer_v<decltype(SCRATCH)>)
        c.scratch_bytes = [](const void *m) -> u64 { return SCRATCH((const typename B::Model *)m, 1); };
    c.sym_bytes = sizeof(typename B::Sym);
    return c;
}

template <auto BATCH, auto SCRATCH = nullptr>
HostDecodeCall scl_host_decode_call() {
    using B = SclBatch<decltype(BATCH)>;
    HostDecodeCall c = {scl_host_run_dec<BATCH>, nullptr};
    if constexpr (!std::is_null_pointer_v<decltype(SCRATCH)>)
        c.scratch_bytes = [](const void *m) -> u64 { return SCRATCH((const typename B::Model *)m, 1); };
    c.sym_bytes = sizeof(typename B::Sym);
    return c;
}
