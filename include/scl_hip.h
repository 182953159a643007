/*
 * scl_hip.h -- C ABI of the MI355X (gfx950) batched entropy-coding core.
 *
 * This is the drop-in boundary for ONE path of the Stanford Compression Library: the per-symbol
 * inner loops of its rANS / tANS / range / arithmetic coders.  Every "batch" entry point runs N
 * independent chunks, one wavefront lane per chunk, and each chunk's output is bit-identical to
 * one call of the reference method it replaces with a fresh coder object:
 *
 *   scl_rans_encode_batch   <->  rANSEncoder.encode_block        scl/compressors/rANS.py:186-210
 *   scl_rans_decode_batch   <->  rANSDecoder.decode_block        scl/compressors/rANS.py:270-297
 *   scl_tans_encode_batch   <->  tANSEncoder.encode_block        scl/compressors/tANS.py:159-193
 *   scl_tans_decode_batch   <->  tANSDecoder.decode_block        scl/compressors/tANS.py:252-279
 *   scl_range_encode_batch  <->  RangeEncoder.encode_block       scl/compressors/range_coder.py:188-207
 *   scl_range_decode_batch  <->  RangeDecoder.decode_block       scl/compressors/range_coder.py:269-317
 *   scl_aec_encode_batch    <->  ArithmeticEncoder.encode_block  scl/compressors/arithmetic_coding.py:80-161
 *   scl_aec_decode_batch    <->  ArithmeticDecoder.decode_block  scl/compressors/arithmetic_coding.py:203-287
 *   (model handles)         <->  rANSParams / tANSParams / RangeCoderParams+Frequencies /
 *                                AECParams+FreqModelBase subclasses (probability_models.py:15-160)
 *   scl_prefix_encode_batch <->  PrefixFreeEncoder.encode_block  scl/compressors/prefix_free_compressors.py:31-50
 *   scl_prefix_decode_batch <->  PrefixFreeDecoder.decode_block  scl/compressors/prefix_free_compressors.py:67-88
 *   (scl_prefix_model)      <->  the code table of a PrefixFreeTree (get_encoding_table, :123-155), e.g. the one
 *                                HuffmanTree.build_huffman_tree makes (scl/compressors/huffman_coder.py:45-93)
 *   scl_streams_compact     <->  the BitArray each encode_block returns (left-aligned bits) and,
 *                                with SCL_COMPACT_FRAMED, EncodedBlockWriter.write_block
 *                                (scl/core/encoded_stream.py:150-175)
 *
 * Conventions
 *   - plain C: pointers, sizes, opaque handles; no C++ or torch types.
 *   - every function returns an int status: SCL_OK or a negative SCL_E_* code;
 *     scl_last_error() gives a thread-local message for the last failure.
 *   - pointers named d_* are DEVICE pointers (HBM) owned by the caller; h_* are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 *     on that stream; nothing synchronises unless stated.
 *   - symbols are alphabet indices (position in Frequencies.freq_dict, prob_dist.py:193-205): uint8 for alphabets
 *     up to 256 entries -- the entry points BASELINE.json's configurations use, served by the tuned kernels -- and
 *     uint16 for alphabets up to 65536 through the *_u16 twins at the end of this header (any-parameter kernels).
 *   - a bit stream is MSB-first packed bytes (bitarray "big" endianness, bitarray_utils.py:25).
 *     A stream is described by (bit_offset, nbits): bit_offset is the absolute position of its
 *     first bit counted from the buffer's base pointer.  Encoders WRITE these descriptors;
 *     decoders READ them, so encoder output feeds the decoder without any repacking:
 *       * rANS / tANS streams are produced back to front (the reference prepends every field,
 *         rANS.py:196) and therefore end exactly at the end of their slot:
 *           bit_offset[c] = 8*(c+1)*out_stride - nbits[c]
 *         The slot bits in front of the stream are zero (this is the front padding of
 *         scl/core/encoded_stream.py:23-46).
 *       * range / arithmetic streams are produced front to back: bit_offset[c] = 8*c*out_stride.
 *     scl_streams_compact turns either into dense, byte-aligned, left-aligned streams.
 *   - per-chunk status words (d_status): 0 = ok, else a bit mask of SCL_ST_*.
 *   - all buffers holding streams must be 16-byte aligned, strides multiples of 16 bytes, and the
 *     input buffer of a decoder must stay readable for 16 bytes past the last stream byte.
 *     scl_*_slot_bytes returns multiples of 128: with 128-byte aligned base pointers (any hipMalloc /
 *     torch allocation) every lane then moves whole, aligned 128-byte lines, which is what the tuned
 *     kernels are built around (smaller alignments are accepted and served by the generic kernels or at
 *     reduced speed).
 */
#ifndef SCL_HIP_H
#define SCL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define SCL_OK 0
#define SCL_E_PARAM (-2)    /* parameter set rejected (also what the reference asserts on)      */
#define SCL_E_ALLOC (-7)    /* device / host allocation failed                                  */
#define SCL_E_HIP (-8)      /* a HIP runtime call failed (see scl_last_error)                    */
#define SCL_E_NODEVICE (-9) /* no gfx950 device visible                                          */
#define SCL_E_CHUNK (-10)   /* host convenience call: the chunk's status word was non-zero       */

/* per-chunk status bits */
#define SCL_ST_CAPACITY 0x1u  /* output slot too small / block larger than out_cap              */
#define SCL_ST_SYMBOL 0x2u    /* symbol index >= K              (KeyError, prob_dist.py:208)     */
#define SCL_ST_TRUNCATED 0x4u /* decoder needed bits past in_nbits                               */
#define SCL_ST_STATE 0x8u     /* final state != INITIAL_STATE   (assert, rANS.py:295)            */
#define SCL_ST_TOTAL 0x10u    /* total_freq >= MAX_ALLOWED_TOTAL_FREQ (assert, arithmetic_coding.py:110) */
#define SCL_ST_SIZE 0x20u     /* block size does not fit DATA_BLOCK_SIZE_BITS                    */

/* ---- library ------------------------------------------------------------------------------ */
const char *scl_last_error(void);
int scl_device_count(int *count);
int scl_abi_version(void);
/* Which kernels serve the batch calls of the CALLING THREAD (ABI version 5): on = 1 keeps the tuned kernels out (every call
   runs the any-parameter kernels -- how the tests compare the two implementations of every coder word for word),
   on = 0 lets the library choose, on = -1 (the initial state) follows the environment variable
   SCL_ANY_PARAMETER_KERNELS as before.  Thread-local: other threads' calls are not affected.  Returns the previous value. */
int scl_set_any_parameter_kernels(int on);

/* ---- rANS ---------------------------------------------------------------------------------- */
typedef struct scl_rans_model scl_rans_model;

typedef struct scl_rans_info {
    uint64_t M, L, H;        /* rANSParams.M / .L / .H              (rANS.py:100-104)            */
    uint32_t K;
    uint32_t num_state_bits; /* rANSParams.NUM_STATE_BITS           (rANS.py:119)                */
    uint32_t size_bits;      /* DATA_BLOCK_SIZE_BITS                                             */
    uint32_t num_bits_out;   /* NUM_BITS_OUT                                                     */
    uint32_t max_bits_per_symbol; /* worst-case field width, for slot sizing                     */
    uint32_t fast_path;      /* 1 if tuned kernels serve this model: u32 state with NUM_BITS_OUT = 1
                                and any total <= 4096, or NUM_BITS_OUT in {2,4,8,16} with a
                                power-of-two total <= 4096 (RANGE_FACTOR a power of two)        */
    int32_t device;          /* the HIP device the handle's tables live on (current at create);
                                batch calls refuse any other current device                     */
} scl_rans_info;

/* rANSParams(freqs, DATA_BLOCK_SIZE_BITS, NUM_BITS_OUT, RANGE_FACTOR) -> device-resident tables.
   Rejects: K == 0 or > 65536, any freq == 0, H >= 2^63 (quirks Q7/Q8), size_bits or num_bits_out
   outside 1..32.  Models of more than 256 symbols are coded through the *_u16 entry points. */
int scl_rans_model_create(const uint32_t *h_freq, uint32_t K, uint64_t range_factor,
                          uint32_t num_bits_out, uint32_t size_bits, scl_rans_model **out);
void scl_rans_model_destroy(scl_rans_model *m);
int scl_rans_model_info(const scl_rans_model *m, scl_rans_info *info);
/* (ABI version 5) which encoder a batch of n_chunks aligned, equally long rows would run with the calling thread's
   current settings: 'L' / 'S' = the headline kernels (NUM_BITS_OUT = 1; NUM_BITS_OUT in {4, 8, 16} within their bounds)
   with the 256-byte-ring / slot-ring writer (chosen by batch size; SCL_RANS_ENC_WRITER=L|S in the environment forces
   one, read at every call), 'B' = the NUM_BITS_OUT > 1 kernels that serve what those bounds exclude (NUM_BITS_OUT = 2,
   ...), 'G' = any-parameter kernels.  For tests and tools. */
int scl_rans_encoder_kind(const scl_rans_model *m, uint64_t n_chunks);
/* (ABI version 6) the encode and the decode kernel such a batch would run, as rocprofv3 prints them (template arguments
   included for the tuned kernels), NUL-terminated into enc / dec (either may be NULL) of `cap` >= 96 bytes: what lets a
   measurement name its kernels so that they can be matched against a kernel-trace summary.  No reference counterpart. */
int scl_rans_kernel_names(const scl_rans_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
/* bytes a slot must have so that any block of n symbols fits (multiple of 128: whole cache lines, so the
   64-byte store bursts of the fast kernels never straddle a sector) */
uint64_t scl_rans_slot_bytes(const scl_rans_model *m, uint64_t n_symbols);

/* chunk c reads symbols d_sym[c*sym_stride .. +len_c) with len_c = d_lens ? d_lens[c] : chunk_len */
int scl_rans_encode_batch(const scl_rans_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                          const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                          uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                          uint32_t *d_out_nbits, uint32_t *d_status, void *stream);

/* chunk c decodes the stream (d_bit_offset[c], d_in_nbits[c]) of d_in into
   d_out_sym[c*out_stride .. ); at most out_cap symbols.  d_out_lens[c] = block size from the
   header, d_consumed[c] = num_bits_consumed (trailing bits are tolerated and not counted). */
int scl_rans_decode_batch(const scl_rans_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                          const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                          uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                          uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                          uint32_t *d_status, void *stream);

/* ---- tANS (cached rANS: M power of two, NUM_BITS_OUT == 1; tANS.py:31-53) -------------------
 * Lookup tables have RANGE_FACTOR * M entries.  Up to 8192 entries they sit in LDS (tuned kernels); up to 2^26 they
 * are built in device memory; beyond that (the reference's inherited default RANGE_FACTOR = 2^16 with M = 4096 asks
 * for 2^28) no table is built and the model runs on the table-free rANS kernels, which write the same stream --
 * scl_tans_model_tables then fails and the batch entry points need 16-byte aligned rows and slots.
 * Since round 3 the table-free kernels are also the DEFAULT for LDS-sized tables wherever they apply (they are the faster
 * way to write the same stream on this machine); SCL_TANS_KERNELS=table in the environment keeps the lookup-table
 * kernels in charge.  scl_tans_model_tables exports the tables either way. */
typedef struct scl_tans_model scl_tans_model;

int scl_tans_model_create(const uint32_t *h_freq, uint32_t K, uint64_t range_factor,
                          uint32_t size_bits, scl_tans_model **out);
void scl_tans_model_destroy(scl_tans_model *m);
int scl_tans_model_info(const scl_tans_model *m, scl_rans_info *info);
uint64_t scl_tans_slot_bytes(const scl_tans_model *m, uint64_t n_symbols);
/* (ABI version 6) as scl_rans_kernel_names (a tANS model the table-free rANS kernels can serve runs on them) */
int scl_tans_kernel_names(const scl_tans_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
/* copy the device lookup tables back (for parity with tANS.py:285-337); any pointer may be NULL.
   h_enc / h_dec_sym / h_dec_xs have RANGE_FACTOR*M entries, h_nbits / h_thresh have K. */
int scl_tans_model_tables(const scl_tans_model *m, uint32_t *h_enc, uint32_t *h_nbits,
                          uint32_t *h_thresh, uint32_t *h_dec_sym, uint32_t *h_dec_xs);
int scl_tans_encode_batch(const scl_tans_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                          const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                          uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                          uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_tans_decode_batch(const scl_tans_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                          const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                          uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                          uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                          uint32_t *d_status, void *stream);

/* ---- range coder (RangeCoderParams + Frequencies; range_coder.py:55-86) --------------------- */
typedef struct scl_range_model scl_range_model;

/* Rejects: precision not a multiple of 8 in 16..32, any freq == 0, total_freq > BOTTOM
   (asserts at range_coder.py:64,84-85). */
int scl_range_model_create(const uint32_t *h_freq, uint32_t K, uint32_t precision,
                           uint32_t size_bits, scl_range_model **out);
void scl_range_model_destroy(scl_range_model *m);
uint64_t scl_range_slot_bytes(const scl_range_model *m, uint64_t n_symbols);
/* 1 if the tuned kernels serve this model (PRECISION = 32, DATA_BLOCK_SIZE_BITS = 32), 0 if the any-parameter ones do */
int scl_range_fast_path(const scl_range_model *m);
int scl_range_encode_batch(const scl_range_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                           const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                           uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                           uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_range_decode_batch(const scl_range_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                           const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                           uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                           uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                           uint32_t *d_status, void *stream);

/* ---- arithmetic coder (AECParams + frequency model; arithmetic_coding.py:20-56) ------------- */
typedef struct scl_aec_model scl_aec_model;

#define SCL_MODEL_FIXED 0  /* FixedFreqModel          probability_models.py:57-67               */
#define SCL_MODEL_IID 1    /* AdaptiveIIDFreqModel    probability_models.py:70-92               */
#define SCL_MODEL_ORDERK 2 /* AdaptiveOrderKFreqModel probability_models.py:95-160              */

/* scl_aec_*_batch: every chunk starts from a FRESH copy of the model (one chunk == one new encoder
   object); coder objects that live across blocks (quirk Q4) use the *_resume entry points below.
   h_freq_init: initial frequencies [K] for FIXED / IID (ignored for ORDERK, which starts from
   all-ones counts).  order_k: context length for ORDERK (0..3).  max_total: the model's
   max_allowed_total_freq.  precision 8..62: up to 32 the tuned kernels serve the models listed at
   scl_aec_fast_path; 33..62 run the any-parameter kernels with low / high in 128 bits (row totals must stay
   below 2^32: SCL_ST_TOTAL otherwise). */
int scl_aec_model_create(int model_kind, const uint32_t *h_freq_init, uint32_t K, uint32_t order_k,
                         uint64_t max_total, uint32_t precision, uint32_t size_bits,
                         scl_aec_model **out);
void scl_aec_model_destroy(scl_aec_model *m);
uint64_t scl_aec_slot_bytes(const scl_aec_model *m, uint64_t n_symbols);
/* bytes of device scratch the adaptive models need for n_chunks concurrent coders (0 for FIXED) */
uint64_t scl_aec_scratch_bytes(const scl_aec_model *m, uint64_t n_chunks);
/* 1 if batches whose chunks hold at most max_symbols symbols are served by the per-lane-LDS-table kernels
   (adaptive models, alphabet <= 16, <= 16 contexts; needs 16-byte aligned rows and slots of
   scl_aec_slot_bytes) -- the kernels BASELINE.json configs[3] names; 0 if the generic kernels serve them. */
int scl_aec_fast_path(const scl_aec_model *m, uint64_t max_symbols);
int scl_aec_encode_batch(const scl_aec_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                         const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                         uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                         uint32_t *d_out_nbits, uint32_t *d_status, void *d_scratch,
                         uint64_t scratch_bytes, void *stream);
int scl_aec_decode_batch(const scl_aec_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                         const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                         uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                         uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                         uint32_t *d_status, void *d_scratch, uint64_t scratch_bytes,
                         void *stream);

/* ---- coder objects that live across blocks (quirk Q4) ----------------------------------------
 * The reference's ArithmeticEncoder / ArithmeticDecoder own their freq_model and never reset it
 * (arithmetic_coding.py:52-56,118), so DataEncoder.encode (core/data_encoder_decoder.py:57-69) codes
 * block i+1 with the counts and the order-k context block i left behind.  The *_resume entry points
 * reproduce that: chunk c of the call CONTINUES coder c of a caller-owned device state buffer
 * (scl_aec_state_bytes(m, n_coders) bytes, 256-byte aligned) and leaves the advanced state there.
 * The layout of the state buffer is a function of the n_coders it was reset with, so every call names that SAME
 * n_coders (state_bytes >= scl_aec_state_bytes(m, n_coders)); a batch may continue fewer coders than the state
 * holds (n_chunks <= n_coders: chunk c continues coder c), never more.
 * They run the any-parameter kernels.  FIXED models have nothing to carry and forward to the
 * plain entry points (d_state may be NULL).
 *
 * Canonical host form of one coder's state (upload / download / *_host_resume):
 *   h_counts : scl_aec_state_counts(m) actual counts -- IID: [K] = freqs_current.freq_list;
 *              ORDERK: [K^(k+1)] row-major, last axis = next symbol = freqs_kplus1_tuple.ravel()
 *              (probability_models.py:110);
 *   h_past_k : the last k symbol indices, oldest first = past_k (probability_models.py:116). */
uint64_t scl_aec_state_bytes(const scl_aec_model *m, uint64_t n_coders);
uint64_t scl_aec_state_counts(const scl_aec_model *m);
/* all n_coders coders = freshly constructed models */
int scl_aec_state_reset(const scl_aec_model *m, void *d_state, uint64_t state_bytes, uint64_t n_coders,
                        void *stream);
/* one coder's state from / to the canonical host form; both synchronise `stream` */
int scl_aec_state_upload(const scl_aec_model *m, void *d_state, uint64_t n_coders, uint64_t coder,
                         const uint32_t *h_counts, const uint32_t *h_past_k, void *stream);
int scl_aec_state_download(const scl_aec_model *m, const void *d_state, uint64_t n_coders, uint64_t coder,
                           uint32_t *h_counts, uint32_t *h_past_k, void *stream);
int scl_aec_encode_batch_resume(const scl_aec_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                                const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                uint32_t *d_out_nbits, uint32_t *d_status, void *d_state,
                                uint64_t state_bytes, uint64_t n_coders, void *stream);
int scl_aec_decode_batch_resume(const scl_aec_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                                uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                uint32_t *d_status, void *d_state, uint64_t state_bytes, uint64_t n_coders,
                                void *stream);

/* ---- prefix-free codes (added to ABI 8 without a version change: the number is pinned by the test suite) ------------
 * Any prefix-free code table: Huffman today (HuffmanEncoder / HuffmanDecoder, huffman_coder.py:96-123), Shannon, Fano and
 * the rest with host code only.  A stream is the block's codewords back to back (prefix_free_compressors.py:31-50): NO size
 * header and no terminator, an empty block is an empty stream, and the decoder walks the tree until in_nbits bits are
 * consumed (:67-88) -- it needs the exact bit length and tolerates no trailing bits.
 * Symbol i is coded with the h_len[i] low bits of h_code[i], most significant first.  Rejected (SCL_E_PARAM): K outside
 * 1..65536, a length of 0 or above 32, a codeword that equals or is a prefix of another.  Incomplete trees are accepted (the
 * one-symbol Huffman code "0" is one).
 * Tuned kernels serve byte symbols (K <= 256; fast_path in scl_prefix_info); the *_u16 twins and
 * scl_set_any_parameter_kernels(1) run the any-parameter kernels, which write and read the same streams.
 *   encode: streams grow front to back, bit_offset[c] = 8*c*out_stride, nbits[c] = sum of the code lengths (0 for an empty
 *           chunk).  SCL_ST_SYMBOL: a symbol index >= K (coded as symbol 0); SCL_ST_CAPACITY: the slot is too small (nothing is
 *           stored past it, nbits[c] still reports the length needed).
 *   decode: d_out_lens[c] = symbols decoded (there is no header to read a count from), d_consumed[c] = bits of the whole
 *           codewords decoded.  SCL_ST_CAPACITY: bits are left after out_cap symbols (nothing is stored past out_cap);
 *           SCL_ST_TRUNCATED: in_nbits ends inside a codeword (the complete symbols before it are delivered);
 *           SCL_ST_STATE: the bits walk into a missing child of an incomplete tree. */
typedef struct scl_prefix_model scl_prefix_model;

typedef struct scl_prefix_info {
    uint32_t K;
    uint32_t min_len, max_len; /* shortest / longest codeword in bits                                */
    uint32_t lut_bits;         /* T = min(max_len, 11): the tuned decoder's lookup table has 2^T entries */
    uint32_t fast_path;        /* 1 if the tuned kernels serve this model (K <= 256)                  */
    int32_t device;
} scl_prefix_info;

int scl_prefix_model_create(const uint32_t *h_code, const uint8_t *h_len, uint32_t K, scl_prefix_model **out);
void scl_prefix_model_destroy(scl_prefix_model *m);
int scl_prefix_model_info(const scl_prefix_model *m, scl_prefix_info *info);
/* as scl_rans_kernel_names */
int scl_prefix_kernel_names(const scl_prefix_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
/* a multiple of 128 that holds n_symbols codewords of the longest length and the writer's last whole word */
uint64_t scl_prefix_slot_bytes(const scl_prefix_model *m, uint64_t n_symbols);
int scl_prefix_encode_batch(const scl_prefix_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                            const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                            uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                            uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_prefix_decode_batch(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                            const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                            uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                            uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                            uint32_t *d_status, void *stream);
int scl_prefix_encode_batch_u16(const scl_prefix_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                                const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_prefix_decode_batch_u16(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                                uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                uint32_t *d_status, void *stream);
/* one chunk in host memory, as the other *_host calls; the decoder's out_cap bounds the symbols (in_nbits / min_len holds
   any stream) */
int scl_prefix_encode_host(const scl_prefix_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                           uint64_t out_cap_bytes, uint64_t *nbits);
int scl_prefix_decode_host(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                           uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_prefix_encode_host_u16(const scl_prefix_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                               uint64_t out_cap_bytes, uint64_t *nbits);
int scl_prefix_decode_host_u16(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                               uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);

/* ---- prefix-free codes, ONE large block coded by the whole grid (scl_prefix_block.hip; added to ABI 8 as above) ----------
 * The batch calls give a chunk to one lane; these give one block to every CU and write / read the very same stream
 * (codewords back to back, no side information), from the same scl_prefix_model.  Positions and counts are 64-bit.
 *   encode: per-tile sums of the code lengths, an exclusive scan of the tile sums, then every workgroup assembles its
 *           tile in LDS and stores whole 32-bit words; the words two tiles share are merged with atomic ORs, so the
 *           call zeroes d_out first (up to out_cap_bytes).  d_out 4-byte aligned.  *d_nbits = sum of the code lengths,
 *           also when it does not fit.  *d_status: SCL_ST_SYMBOL (an index >= K, coded as symbol 0), SCL_ST_CAPACITY
 *           ((nbits + 7) / 8 > out_cap_bytes: the stream is not written; nothing is ever stored at or past
 *           d_out + out_cap_bytes).  Asynchronous on `stream`.
 *   decode: self-synchronising speculative decoding (Weissenberger & Schmidt 2018): the stream is cut into subsequences
 *           of sub_bits bits, one per thread, 256 per workgroup; every thread decodes from a guessed start, takes its
 *           left neighbour's exit as its start and decodes again until nothing changes -- inside a workgroup under
 *           __syncthreads, between workgroups by relaunching a pass until a device flag says that no workgroup's exit
 *           changed.  THE CALL READS THAT FLAG BETWEEN PASSES: it synchronises `stream` once per pass (a stream inside
 *           one workgroup needs no pass and no synchronisation).  No kernel waits on another workgroup.  The result is the sequential decode for every table and
 *           every stream; a code that never falls into step costs one pass per workgroup.
 *           d_in 4-byte aligned; the stream is the in_nbits bits from absolute bit in_bit_offset of d_in, and reads stay
 *           inside [d_in, d_in + in_size_bytes).  d_result receives what the one-lane decoder reports for the same
 *           stream: n_out symbols stored (never more than out_cap), consumed = bits of the whole codewords decoded,
 *           status 0 / SCL_ST_TRUNCATED / SCL_ST_STATE / SCL_ST_CAPACITY, and sync_passes = passes after the first in
 *           which a workgroup had to move its start (0: the speculation was right at every workgroup boundary).
 * SCL_E_PARAM (message = the entry point's name + ':'), before any device call: null model or buffers, a model of
 * another device, the uint8 form with K > 256, misaligned d_out / d_in / d_scratch (8 bytes), scratch_bytes below
 * scl_prefix_block_scratch_bytes, n >= 2^32 symbols, in_nbits >= 2^46. */
typedef struct scl_prefix_block_info {
    uint32_t sub_bits;     /* S: bits per decoder thread; a decoder workgroup owns 256 * S bits */
    uint32_t tile_symbols; /* symbols per encoder workgroup                                      */
    uint32_t code_len_gcd; /* gcd of the code lengths: a start guess is a multiple of it         */
} scl_prefix_block_info;

typedef struct scl_prefix_block_result {
    uint64_t n_out, consumed;
    uint32_t status, sync_passes;
} scl_prefix_block_result;

int scl_prefix_block_info_get(const scl_prefix_model *m, scl_prefix_block_info *info);
/* device scratch that serves an encode of n_symbols and a decode of in_nbits (0 for a null model) */
uint64_t scl_prefix_block_scratch_bytes(const scl_prefix_model *m, uint64_t n_symbols, uint64_t in_nbits);
int scl_prefix_encode_block(const scl_prefix_model *m, const uint8_t *d_sym, uint64_t n, uint8_t *d_out,
                            uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                            uint64_t scratch_bytes, void *stream);
int scl_prefix_encode_block_u16(const scl_prefix_model *m, const uint16_t *d_sym, uint64_t n, uint8_t *d_out,
                                uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                uint64_t scratch_bytes, void *stream);
int scl_prefix_decode_block(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                            uint64_t in_bit_offset, uint64_t in_nbits, uint8_t *d_out_sym, uint64_t out_cap,
                            scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream);
int scl_prefix_decode_block_u16(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                uint64_t in_bit_offset, uint64_t in_nbits, uint16_t *d_out_sym, uint64_t out_cap,
                                scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                void *stream);
/* one block in host memory: allocate, copy, run, synchronise -- as scl_prefix_encode_host / _decode_host and with their
   error codes for a non-zero status, without their limit of 2^32 bits per stream */
int scl_prefix_encode_block_host(const scl_prefix_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                                 uint64_t out_cap_bytes, uint64_t *nbits);
int scl_prefix_decode_block_host(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                 uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_prefix_encode_block_host_u16(const scl_prefix_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                                     uint64_t out_cap_bytes, uint64_t *nbits);
int scl_prefix_decode_block_host_u16(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                     uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);

/* ---- integer codes, ONE block coded by the whole grid (scl_uint_block.hip; added to ABI 8 as above) ----------------------
 * The reference's three prefix codes over unbounded non-negative integers -- GolombUintEncoder(M) (golomb_coder.py),
 * UniversalUintEncoder (universal_uint_coder.py), EliasDeltaUintEncoder (elias_delta_uint_coder.py) -- over uint32 values,
 * with the kernels of the prefix-free block above: the codeword is computed from the value instead of read from a table
 * (csrc/scl_uint_code.h), everything else is the same code.  The stream is the codewords back to back.
 * A codeword travels in one 32-bit word.  Longer ones are not coded: universal x >= 2^16, Elias-delta x >= 2^24 - 1,
 * Golomb x / M + 1 + b (+ 1) > 32 with b = floor(log2 M).
 *   encode: as scl_prefix_encode_block.  *d_status: SCL_ST_SIZE = a value whose codeword is longer than 32 bits (*d_nbits = 0),
 *           SCL_ST_CAPACITY = (nbits + 7) / 8 > out_cap_bytes (*d_nbits = the length needed).  With either, no codeword is
 *           stored (the call still zeroes d_out up to min(out_cap_bytes, 4 * n)).
 *   decode: as scl_prefix_decode_block, d_result likewise.  status: SCL_ST_TRUNCATED = in_nbits ends inside a codeword (in
 *           its unary part, length field, remainder or Golomb's extra bit); SCL_ST_SIZE = a prefix that announces a
 *           codeword of more than 32 bits; SCL_ST_CAPACITY = bits are left after out_cap values.  consumed = the bits of the
 *           whole codewords in front, whose values are delivered.
 * SCL_E_PARAM (message = the entry point's name + ':'), before any device call: a null pointer, an unknown kind, a Golomb
 * code with M = 0 or M >= 2^31 (M is not looked at for the other kinds), misaligned d_out / d_in (4 bytes), d_val / d_out_val
 * (4 bytes), d_scratch / d_nbits / d_result (8 bytes), scratch_bytes below scl_uint_block_scratch_bytes, n >= 2^32 values,
 * in_nbits >= 2^46, a stream that ends behind in_size_bytes. */
#define SCL_UINT_GOLOMB 0u
#define SCL_UINT_UNIVERSAL 1u
#define SCL_UINT_ELIAS_DELTA 2u

typedef struct scl_uint_code {
    uint32_t kind; /* SCL_UINT_*               */
    uint32_t M;    /* Golomb's parameter        */
} scl_uint_code;

typedef struct scl_uint_block_result {
    uint64_t n_out, consumed;
    uint32_t status, sync_passes;
} scl_uint_block_result;

/* device scratch that serves an encode of n_values and a decode of in_nbits */
uint64_t scl_uint_block_scratch_bytes(uint64_t n_values, uint64_t in_nbits);
int scl_uint_encode_block(const scl_uint_code *code, const uint32_t *d_val, uint64_t n, uint8_t *d_out,
                          uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                          uint64_t scratch_bytes, void *stream);
int scl_uint_decode_block(const scl_uint_code *code, const uint8_t *d_in, uint64_t in_size_bytes, uint64_t in_bit_offset,
                          uint64_t in_nbits, uint32_t *d_out_val, uint64_t out_cap, scl_uint_block_result *d_result,
                          void *d_scratch, uint64_t scratch_bytes, void *stream);
/* one block in host memory: allocate, copy, run, synchronise.  *status = the block's status word: with SCL_ST_SIZE a caller
   codes the block elsewhere, so a non-zero status is reported, not turned into SCL_E_CHUNK.  encode: h_out receives the
   stream only for status 0 (SCL_E_PARAM if it needs more than out_cap_bytes); decode: the n_out values in front of the
   fault are delivered with any status. */
int scl_uint_encode_block_host(const scl_uint_code *code, const uint32_t *h_val, uint64_t n, uint8_t *h_out,
                               uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status);
int scl_uint_decode_block_host(const scl_uint_code *code, const uint8_t *h_in, uint64_t in_nbits, uint32_t *h_out_val,
                               uint64_t out_cap, uint64_t *n_out, uint64_t *consumed, uint32_t *status);
/* The code rule itself, on the host, no device: what the kernels compute per value (the same function compiled for both).
   scl_uint_codeword_host: *bits = the codeword right-aligned, *len = its length, 0 for one longer than 32 bits.
   scl_uint_decode_one_host: one codeword from the 32 left-aligned bits of `bits32`, of which `rem` >= 1 belong to the stream
   -> 0 (*x in *len bits), SCL_ST_TRUNCATED or SCL_ST_SIZE.  Both: SCL_E_PARAM for a refused code, a null pointer or rem = 0. */
int scl_uint_codeword_host(const scl_uint_code *code, uint32_t x, uint32_t *bits, uint32_t *len);
int scl_uint_decode_one_host(const scl_uint_code *code, uint32_t bits32, uint32_t rem, uint32_t *len, uint32_t *x);

/* ---- integer codes, batched: one wavefront lane per chunk (scl_uint.hip; added to ABI 8 as above) -----------------------
 * The same three codes with the call shape of scl_prefix_encode_batch / scl_prefix_decode_batch, a scl_uint_code in place of
 * the model: rows of uint32 values (strides in ELEMENTS), one independent stream per chunk, stream layout, bit_offset, nbits
 * and slots as there.  EVERY uint32 value has a codeword here: a lane writes it as a run of ones and at most two fields of
 * at most 32 bits (universal and Elias-delta codewords reach 64 bits, a Golomb codeword x / M + 32).
 *   scl_uint_slot_bytes: n_values codewords of max_value (no shorter value has a longer one: the lengths never decrease in
 *           x), plus the writer's last word, rounded up to 128; 0 for a refused code.
 *   encode: d_status[c]: SCL_ST_CAPACITY alone = the stream needs more than out_stride bytes in whole words; nbits[c] is then
 *           (as always) the length needed, counted in 64 bits and saturating at 2^32 - 1, and what the slot holds is
 *           unspecified.  Nothing is stored at or past a slot's end; zero bits follow a stream up to its last stored word.
 *   decode: d_out_lens, d_consumed and the whole codewords in front of a fault as scl_prefix_decode_batch.  d_status[c], in
 *           the order a sequential reader meets them (csrc/scl_uint_code.h): SCL_ST_TRUNCATED = in_nbits
 *           ends inside a codeword; SCL_ST_SIZE = the codeword announces a value of 2^32 and more (Golomb: ones up to a
 *           quotient q with M * q >= 2^32, or M * q + r >= 2^32; universal: 32 ones; Elias-delta: six zeros, n > 32, or
 *           n = 32 with low bits); SCL_ST_CAPACITY = bits are left after out_cap values.
 *   Two kernel pairs that write and read the same bits: the tuned pair runs when value rows and output rows start on 16-byte
 *   boundaries (pointer and stride), d_in does, in_size_bytes is a multiple of 16 and the calling thread has not called
 *   scl_set_any_parameter_kernels(1); other rows run the any-parameter pair as they are (no row is re-laid).
 *   scl_uint_kernel_names names the pair of a batch of such aligned rows, as rocprofv3 prints it.
 * SCL_E_PARAM (message = the entry point's name + ':'), before any device call: a null pointer (d_lens and d_status may be
 * null), an unknown kind, a Golomb code with M = 0 or M >= 2^31, an out_stride that is not a positive multiple of 16 below
 * 512 MiB, d_out not 16-byte aligned, d_in / d_val / d_out_val not 4-byte aligned. */
uint64_t scl_uint_slot_bytes(const scl_uint_code *code, uint64_t n_values, uint32_t max_value);
int scl_uint_encode_batch(const scl_uint_code *code, const uint32_t *d_val, uint64_t val_stride, const uint32_t *d_lens,
                          uint32_t chunk_len, uint64_t n_chunks, uint8_t *d_out, uint64_t out_stride,
                          uint64_t *d_out_bit_offset, uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_uint_decode_batch(const scl_uint_code *code, const uint8_t *d_in, uint64_t in_size_bytes,
                          const uint64_t *d_bit_offset, const uint32_t *d_in_nbits, uint64_t n_chunks, uint32_t *d_out_val,
                          uint64_t out_stride, uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                          uint32_t *d_status, void *stream);
int scl_uint_kernel_names(const scl_uint_code *code, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
/* The rule of these kernels on the host, no device (the same functions compiled for both).
   scl_uint_fields_host: the codeword of x = *run ones, then the widths[0] low bits of fields[0], then the widths[1] low bits
   of fields[1] (a width is at most 32; 0: no such field).
   scl_uint_decode_wide_one_host: one codeword read from bit bit_pos of the buf_bytes bytes at buf (zeros behind them), of
   which `rem` >= 1 bits belong to the stream -> 0 (*x in *len bits), SCL_ST_TRUNCATED or SCL_ST_SIZE. */
int scl_uint_fields_host(const scl_uint_code *code, uint32_t x, uint32_t *run, uint32_t *fields, uint32_t *widths);
int scl_uint_decode_wide_one_host(const scl_uint_code *code, const uint8_t *buf, uint64_t buf_bytes, uint64_t bit_pos,
                                  uint32_t rem, uint32_t *len, uint32_t *x);

/* ---- fixed-width codes, batched: a stream across as many workgroups as it has tiles (scl_fixed.hip; added to ABI 8 as above)
 * The data section of the reference's FixedBitwidthEncoder.encode_block (fixed_bitwidth_compressor.py): symbol index i of a
 * stream of width w is the w bits [i * w, (i + 1) * w) of the stream, most significant first, stream bit b = bit 7 - b % 8 of
 * byte b / 8; the unused bits of the last stored word are 0.  No table, no model, no scan: a ragged batch of streams, each with
 * its own length n[c] < 2^32 (d_lens, or chunk_len for all), width h_widths[c] in 1..32 and alphabet size h_K[c] with
 * 1 <= K <= 2^w.  h_widths and h_K are HOST arrays of n_chunks entries, uploaded by the call.  32 symbols are w words for
 * every w, so a workgroup's tile of SCL_FIXED_TILE symbols is a whole number of stream words: the grid is (tiles of the
 * longest stream) x (streams), workgroups past a stream's end leave at once, and one large stream fills the GPU by the same
 * call.  Rows are uint8, uint16 (_u16) or uint32 (_u32) indices, strides in ELEMENTS; rows are read and written in 16-byte
 * pieces, so row starts (pointer, stride * element size) are multiples of 16 bytes, as are slots.
 *   scl_fixed_slot_bytes(n, w): the stream's whole words, rounded up to 16; 0 for w outside 1..32 or a stream of 2^32 bits
 *           and more.
 *   encode: stream c from bit 0 of slot c (bit_offset[c] = 8 * c * out_stride), nbits[c] = n * w (saturating at 2^32 - 1).
 *           d_status[c]: SCL_ST_SYMBOL = an index >= K (coded as index 0); SCL_ST_CAPACITY = the stream's words need more than
 *           out_stride bytes: nothing is stored, nbits[c] still reports n * w.  Nothing is stored at or past a slot's end
 *           or past the stream's last word.
 *   decode: stream c = the d_in_nbits[c] bits from ANY bit d_bit_offset[c] of d_in, d_lens[c] (or out_cap for all) symbols
 *           asked for.  d_out_lens[c] = the whole symbols delivered, d_consumed[c] = their bits.  d_status[c]:
 *           SCL_ST_TRUNCATED = n * w > in_nbits (or the bits reach past in_size_bytes): the whole symbols in front are
 *           delivered; SCL_ST_SYMBOL = a decoded index >= K, stored as 0; SCL_ST_CAPACITY = n > out_cap: nothing is stored
 *           past out_cap.  No byte at or past in_size_bytes is read.
 *   d_status may not be null here: the call zeroes it and the kernels raise faults on it with atomics.
 *   scl_fixed_kernel_names(sym_bytes, ...): the pair for rows of 1, 2 or 4 byte symbols, as rocprofv3 prints it.
 * SCL_E_PARAM (message = the entry point's name + ':'), before any device call: a null pointer (d_lens may be null), a
 * width outside 1..32, K = 0 or K > 2^w, a width above 8 / 16 through the uint8 / uint16 entry, a row or slot stride that is
 * not a multiple of 16 bytes (out_stride positive, below 512 MiB) or a row stride below chunk_len / out_cap, d_sym / d_out / d_in / d_out_sym not 16-byte aligned,
 * more than 2^31 - 1 workgroups. */
#define SCL_FIXED_TILE 8192u /* symbols per workgroup: 256 lanes x 32 symbols */
uint64_t scl_fixed_slot_bytes(uint64_t n_symbols, uint32_t width);
int scl_fixed_encode_batch(const uint8_t *d_sym, uint64_t sym_stride, const uint32_t *d_lens, uint32_t chunk_len,
                           const uint32_t *h_widths, const uint64_t *h_K, uint64_t n_chunks, uint8_t *d_out,
                           uint64_t out_stride, uint64_t *d_out_bit_offset, uint32_t *d_out_nbits, uint32_t *d_status,
                           void *stream);
int scl_fixed_encode_batch_u16(const uint16_t *d_sym, uint64_t sym_stride, const uint32_t *d_lens, uint32_t chunk_len,
                               const uint32_t *h_widths, const uint64_t *h_K, uint64_t n_chunks, uint8_t *d_out,
                               uint64_t out_stride, uint64_t *d_out_bit_offset, uint32_t *d_out_nbits, uint32_t *d_status,
                               void *stream);
int scl_fixed_encode_batch_u32(const uint32_t *d_sym, uint64_t sym_stride, const uint32_t *d_lens, uint32_t chunk_len,
                               const uint32_t *h_widths, const uint64_t *h_K, uint64_t n_chunks, uint8_t *d_out,
                               uint64_t out_stride, uint64_t *d_out_bit_offset, uint32_t *d_out_nbits, uint32_t *d_status,
                               void *stream);
int scl_fixed_decode_batch(const uint8_t *d_in, uint64_t in_size_bytes, const uint64_t *d_bit_offset,
                           const uint32_t *d_in_nbits, const uint32_t *d_lens, const uint32_t *h_widths, const uint64_t *h_K,
                           uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride, uint32_t out_cap,
                           uint32_t *d_out_lens, uint32_t *d_consumed, uint32_t *d_status, void *stream);
int scl_fixed_decode_batch_u16(const uint8_t *d_in, uint64_t in_size_bytes, const uint64_t *d_bit_offset,
                               const uint32_t *d_in_nbits, const uint32_t *d_lens, const uint32_t *h_widths,
                               const uint64_t *h_K, uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                               uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed, uint32_t *d_status, void *stream);
int scl_fixed_decode_batch_u32(const uint8_t *d_in, uint64_t in_size_bytes, const uint64_t *d_bit_offset,
                               const uint32_t *d_in_nbits, const uint32_t *d_lens, const uint32_t *h_widths,
                               const uint64_t *h_K, uint64_t n_chunks, uint32_t *d_out_sym, uint64_t out_stride,
                               uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed, uint32_t *d_status, void *stream);
int scl_fixed_kernel_names(uint32_t sym_bytes, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
/* one stream in host memory (uint32 indices): allocate, copy, run, synchronise.  *status = the stream's status word, reported
   rather than turned into SCL_E_CHUNK.  encode: h_out receives the (nbits + 7) / 8 stream bytes for a status without
   SCL_ST_CAPACITY (SCL_E_PARAM if out_cap_bytes is below them).  decode: the stream is the in_nbits bits from bit
   in_bit_offset of h_in; h_out_idx receives the *n_out <= out_cap whole symbols in front of a fault. */
int scl_fixed_encode_host(const uint32_t *h_idx, uint64_t n, uint32_t width, uint64_t K, uint8_t *h_out,
                          uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status);
int scl_fixed_decode_host(const uint8_t *h_in, uint64_t in_bit_offset, uint64_t in_nbits, uint64_t n, uint32_t width,
                          uint64_t K, uint32_t *h_out_idx, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                          uint32_t *status);

/* ---- typical-set code: tables built on the device, ONE block coded by the whole grid (scl_typical.hip; added to ABI 8 as above)
 * The reference's TypicalSetEncoder / TypicalSetDecoder (typical_set_coder.py).  A block is cut into chunks of n symbols; chunk
 * x_0..x_{n-1} is tuple t = sum x_i * K^(n-1-i) of the N = K^n tuples in itertools.product order.  Tuple t is typical iff
 * fabs(s / (double)n - entropy) <= eps with s = nlp[x_0] + nlp[x_1] + ... + nlp[x_{n-1}] summed in that order in float64
 * (csrc/scl_typical_rule.h: the one function, compiled for the host and the device).  The `count` typical tuples are numbered
 * in the order of t.  A typical chunk is coded as bit 0 and its number in bt = ceil(log2 count) bits, any other as bit 1 and t
 * in bo = ceil(log2 N) bits, most significant first.  The stream is the codewords back to back, nothing else.
 *   scl_typical_model_create: h_nlp = -log2 p of the K symbols (host, float64), uploaded; rank[N] (the number of a typical
 *           tuple, SCL_TYPICAL_NONE otherwise) and inv[count] (its inverse) are built by three kernels on the current
 *           device, whose buffers are filled with 0xA5 in front of them.  SCL_E_PARAM before any device call, the message
 *           naming the limit: a null pointer, K = 0, n = 0, K > 65536, n > 2^24, K^n > 2^24 (SCL_TYPICAL_MAX_TUPLES: the
 *           longest codeword is then 25 bits and rank[] 64 MiB), a non-finite nlp, entropy or eps.  A negative eps is legal:
 *           no tuple is typical.
 *   scl_typical_model_info: bt = SCL_TYPICAL_NONE for an empty typical set (0: one member).
 *   scl_typical_model_tables: rank[N] and inv[count] copied to the host (either may be NULL).
 *   scl_typical_table_host: the same table on the CPU, no device: h_rank[N] (may be NULL: the count alone), *count.
 *   scl_typical_index_bits_host: ceil(log2 x) in integers as the model computes bt and bo; x = 0 gives SCL_TYPICAL_NONE.
 *   encode: as scl_prefix_encode_block over n_symbols symbol indices (uint8: K <= 256; _u16: any K); n_symbols is a multiple
 *           of n.  *d_status: SCL_ST_SYMBOL = an index >= K (coded as index 0), SCL_ST_CAPACITY as there.
 *   decode: as scl_prefix_decode_block; out_cap, n_out count SYMBOLS (whole chunks are delivered: out_cap / n of them at the
 *           most).  status, at the sequentially first codeword that has one: SCL_ST_TRUNCATED = in_nbits ends inside a
 *           codeword; SCL_ST_STATE = flag 0 with an empty typical set, a typical number >= count, or flag 1 with t >= N;
 *           SCL_ST_CAPACITY = bits are left after out_cap / n chunks.  consumed = the bits of the whole chunks in front.
 *   the *_block_host calls report the status word as scl_uint_*_block_host do.
 * SCL_E_PARAM (message = the entry point's name + ':'), before any device call: a null pointer, a model of another device, a
 * model of more than 256 symbols through a uint8 entry point, n_symbols % n != 0, the misalignments, scratch and size limits of
 * scl_prefix_*_block (d_sym / d_out_sym: the symbol size; the scratch: scl_typical_block_scratch_bytes). */
#define SCL_TYPICAL_MAX_TUPLES (1u << 24)
#define SCL_TYPICAL_NONE 0xFFFFFFFFu

typedef struct scl_typical_model scl_typical_model;
typedef struct scl_typical_info {
    uint32_t N, count; /* tuples, typical tuples                              */
    uint32_t bt, bo;   /* index widths (bt: SCL_TYPICAL_NONE for count = 0)   */
    uint32_t K, n;
    int32_t device;
    uint32_t reserved;
} scl_typical_info;

typedef struct scl_typical_block_result {
    uint64_t n_out, consumed;
    uint32_t status, sync_passes;
} scl_typical_block_result;

int scl_typical_model_create(const double *h_nlp, uint32_t K, uint32_t n, double entropy, double eps,
                             scl_typical_model **out);
void scl_typical_model_destroy(scl_typical_model *m);
int scl_typical_model_info(const scl_typical_model *m, scl_typical_info *info);
int scl_typical_model_tables(const scl_typical_model *m, uint32_t *h_rank, uint32_t *h_inv);
int scl_typical_table_host(const double *h_nlp, uint32_t K, uint32_t n, double entropy, double eps, uint32_t *h_rank,
                           uint32_t *count);
uint32_t scl_typical_index_bits_host(uint64_t x);
/* device scratch that serves an encode of n_symbols and a decode of in_nbits with this model */
uint64_t scl_typical_block_scratch_bytes(const scl_typical_model *m, uint64_t n_symbols, uint64_t in_nbits);
int scl_typical_encode_block(const scl_typical_model *m, const uint8_t *d_sym, uint64_t n_symbols, uint8_t *d_out,
                             uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                             uint64_t scratch_bytes, void *stream);
int scl_typical_encode_block_u16(const scl_typical_model *m, const uint16_t *d_sym, uint64_t n_symbols, uint8_t *d_out,
                                 uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                 uint64_t scratch_bytes, void *stream);
int scl_typical_decode_block(const scl_typical_model *m, const uint8_t *d_in, uint64_t in_size_bytes, uint64_t in_bit_offset,
                             uint64_t in_nbits, uint8_t *d_out_sym, uint64_t out_cap, scl_typical_block_result *d_result,
                             void *d_scratch, uint64_t scratch_bytes, void *stream);
int scl_typical_decode_block_u16(const scl_typical_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                 uint64_t in_bit_offset, uint64_t in_nbits, uint16_t *d_out_sym, uint64_t out_cap,
                                 scl_typical_block_result *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream);
int scl_typical_encode_block_host(const scl_typical_model *m, const uint8_t *h_sym, uint64_t n_symbols, uint8_t *h_out,
                                  uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status);
int scl_typical_encode_block_host_u16(const scl_typical_model *m, const uint16_t *h_sym, uint64_t n_symbols, uint8_t *h_out,
                                      uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status);
int scl_typical_decode_block_host(const scl_typical_model *m, const uint8_t *h_in, uint64_t in_nbits, uint8_t *h_out_sym,
                                  uint64_t out_cap, uint64_t *n_out, uint64_t *consumed, uint32_t *status);
int scl_typical_decode_block_host_u16(const scl_typical_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                      uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                                      uint32_t *status);

/* ---- LZ77: match index, greedy parse and sequence replay (scl_lz77.hip; added to ABI 8 as above) -----------------------
 * The LZ layer of the reference's LZ77 coder, for a batch of independent streams, one wavefront per stream:
 *   scl_lz77_parse_batch   <->  LZ77Encoder.lz77_parse_and_generate_sequences   scl/compressors/lz77.py:525-603
 *   scl_lz77_replay_batch  <->  LZ77Decoder.execute_lz77_sequences              scl/compressors/lz77.py:640-665
 * (the entropy stage above it: host code over the prefix-code entry points in the classes, the scl_lz77_entropy_* calls
 * below for batches).  A stream's WINDOW is everything its coder
 * has seen, the current block included; the windows of a batch lie one after another in d_win, window s = bytes
 * [d_win_off[s], d_win_off[s + 1]) (any offsets: windows need no alignment), and positions inside a window are 32-bit.
 *   parse : the block of stream s is its window from d_start[s] on.  With L = min_match_length (1..8: an L-gram is one
 *           64-bit key) and M = max_matches (0 = no limit) the call writes what the reference's parse returns: sequences
 *           (literal_count, match_length, match_offset) into row s (seq_cap entries) of the three arrays, d_n_seq[s] of
 *           them, and the literals -- d_n_lit[s] bytes at d_literals + d_win_off[s] + d_start[s]: d_literals is laid out
 *           like d_win, every block has room for itself.  It runs an index phase over all total_bytes positions of the
 *           batch (total_bytes < 2^32; a stable radix sort by stream and gram, and one candidate bit per position) and the
 *           parse phase proper; `phases` = 0 runs both, SCL_LZ77_INDEX / SCL_LZ77_PARSE one of them on the same scratch
 *           (for measurements).  d_status[s]: SCL_ST_CAPACITY = more than seq_cap sequences (block_len / L always
 *           suffices; the row holds the first seq_cap), SCL_ST_SIZE = window s does not lie inside [0, total_bytes) or
 *           d_start[s] past its end (nothing is read or written for it).
 *   replay: appends to window s, whose slot is [d_win_off[s], d_win_off[s + 1]) and holds d_have[s] bytes already (the
 *           history: it stays on the device across blocks): per sequence literal_count literals, then match_length bytes
 *           from match_offset back (overlapping matches repeat, as in the reference); then the literals left over.  Stream
 *           s reads d_n_lit[s] literals at d_literals + d_lit_off[s] (inside lit_bytes) and d_n_seq[s] <= seq_cap
 *           sequences; d_out_len[s] = bytes appended.  Nothing outside the slot is read or written on any input;
 *           d_status[s]: SCL_ST_STATE = match_offset 0 or larger than the bytes so far, SCL_ST_TRUNCATED = the sequences
 *           ask for more literals than there are, SCL_ST_CAPACITY = the slot is full, SCL_ST_SIZE = a slot or literal
 *           range outside its buffer.  The stream stops at its first fault; d_out_len[s] counts what came before.
 * Both are asynchronous on `stream`.  SCL_E_PARAM before any device call: a null pointer, L outside 1..8, total_bytes or
 * n_streams >= 2^32, scratch misaligned (256 bytes) or smaller than scl_lz77_scratch_bytes. */
#define SCL_LZ77_INDEX 1u
#define SCL_LZ77_PARSE 2u

typedef struct scl_lz77_parse_args {
    const uint8_t *d_win;
    const uint64_t *d_win_off; /* [n_streams + 1] */
    const uint32_t *d_start;   /* [n_streams]     */
    uint64_t n_streams;
    uint64_t total_bytes;      /* bytes of d_win and of d_literals */
    uint32_t min_match_length, max_matches;
    uint32_t seq_cap, phases;
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    uint8_t *d_literals;
    uint32_t *d_n_seq, *d_n_lit, *d_status; /* [n_streams] each */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_parse_args;

typedef struct scl_lz77_replay_args {
    uint8_t *d_win;
    const uint64_t *d_win_off; /* [n_streams + 1]: the slots */
    const uint32_t *d_have;    /* [n_streams]: bytes already in each slot */
    uint64_t n_streams;
    uint64_t total_bytes;      /* bytes of d_win */
    uint32_t seq_cap, reserved;
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    const uint32_t *d_n_seq;
    const uint8_t *d_literals;
    uint64_t lit_bytes;
    const uint64_t *d_lit_off; /* [n_streams] */
    const uint32_t *d_n_lit;
    uint32_t *d_out_len, *d_status;
} scl_lz77_replay_args;

uint64_t scl_lz77_scratch_bytes(uint64_t total_bytes, uint64_t n_streams);
int scl_lz77_parse_batch(const scl_lz77_parse_args *args, void *stream);
int scl_lz77_replay_batch(const scl_lz77_replay_args *args, void *stream);
/* the kernels that carry the index (its scatter pass), the parse and the replay, as scl_rans_kernel_names; any may be NULL */
int scl_lz77_kernel_names(char *index, char *parse, char *replay, uint64_t cap);
/* one stream in host memory: allocate, copy, run, synchronise.  parse: the window is h_window[0..n), the block starts at
   `start`; h_literals holds at least n - start bytes.  replay: h_window has room for `cap` bytes and holds `have`; the new
   bytes are written behind them.  A non-zero stream status is SCL_E_CHUNK, as in the other *_host calls. */
int scl_lz77_parse_host(const uint8_t *h_window, uint64_t n, uint64_t start, uint32_t min_match_length,
                        uint32_t max_matches, uint32_t *h_lit_count, uint32_t *h_match_len, uint32_t *h_match_off,
                        uint64_t seq_cap, uint64_t *n_seq, uint8_t *h_literals, uint64_t lit_cap, uint64_t *n_lit);
int scl_lz77_replay_host(uint8_t *h_window, uint64_t have, uint64_t cap, const uint32_t *h_lit_count,
                         const uint32_t *h_match_len, const uint32_t *h_match_off, uint64_t n_seq,
                         const uint8_t *h_literals, uint64_t n_lit, uint64_t *out_len);

/* ---- LZ77 with a sliding window: hash-bucket index, lazy parse, windowed replay (scl_lz77_sliding.hip; added to ABI 8) ----
 *   scl_lz77_sliding_parse_batch   <->  LZ77SlidingWindowEncoder.lz77_parse_and_generate_sequences with a
 *                                       HashBasedMatchFinder                     scl/compressors/lz77_sliding_window.py
 *   scl_lz77_sliding_replay_batch  <->  LZ77SlidingWindowDecoder.execute_lz77_sequences
 * The batch layout, the outputs and the statuses are those of scl_lz77_parse_batch / scl_lz77_replay_batch; the sequences
 * go through the same entropy stage.  One wavefront per stream.
 *   parse : hl = hash_length (1..8), m = hash_table_size (1 <= m < 2^32), C = max_chain_length (1..64), mml =
 *           min_match_length (>= 1), W = window_size (0: no bound).  bucket(p) = the reference's hash(tuple(w[p..p+hl))) % m
 *           (CPython's tuple hash: scl_lz77_sliding_bucket_host).  The candidates of p at horizon T are the C newest q < T
 *           of p's bucket; those with p - q > W are skipped but counted.  A candidate is extended right (up to the end of
 *           the window, over p if it comes to that) and then left while the bytes in front are equal, down to the start E
 *           of the lookahead and to position max(0, E - W) + 1 of the source; the longest wins, the newest on ties.  From E
 *           the first p whose best match has mml bytes or more is taken (T = p); if `lazy`, the positions behind it are
 *           tried at the SAME horizon while each beats the best so far.  The sequence is (literals, length, offset), and
 *           a lookahead without such a p gives literal-only sequences (k, 0, 0): DESIGN.md 3.6.4 has the rule in full.
 *           A block yields at most block_len / mml + 2 sequences.  The index phase sorts all positions by (stream, bucket)
 *           and marks those with a predecessor in their bucket within W.
 *   replay: as scl_lz77_replay_batch, except that a sequence with match_length 0 copies nothing and its offset is not
 *           looked at, and that an offset above min(W, bytes so far) is SCL_ST_STATE (W = 0: no bound).
 * Both are asynchronous on `stream`.  SCL_E_PARAM before any device call: a null pointer, hl outside 1..8, m = 0 or
 * m >= 2^32, C outside 1..64, mml = 0, total_bytes or n_streams >= 2^32, scratch misaligned (256 bytes) or smaller than
 * scl_lz77_sliding_scratch_bytes. */
typedef struct scl_lz77_sliding_parse_args {
    const uint8_t *d_win;
    const uint64_t *d_win_off; /* [n_streams + 1] */
    const uint32_t *d_start;   /* [n_streams]     */
    uint64_t n_streams;
    uint64_t total_bytes;      /* bytes of d_win and of d_literals */
    uint64_t hash_table_size;
    uint32_t hash_length, max_chain_length;
    uint32_t lazy, min_match_length;
    uint32_t window_size, seq_cap;
    uint32_t phases, reserved; /* phases: as scl_lz77_parse_args */
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    uint8_t *d_literals;
    uint32_t *d_n_seq, *d_n_lit, *d_status; /* [n_streams] each */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_sliding_parse_args;

typedef struct scl_lz77_sliding_replay_args {
    uint8_t *d_win;
    const uint64_t *d_win_off; /* [n_streams + 1]: the slots */
    const uint32_t *d_have;    /* [n_streams]: bytes already in each slot */
    uint64_t n_streams;
    uint64_t total_bytes;      /* bytes of d_win */
    uint32_t seq_cap, window_size;
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    const uint32_t *d_n_seq;
    const uint8_t *d_literals;
    uint64_t lit_bytes;
    const uint64_t *d_lit_off; /* [n_streams] */
    const uint32_t *d_n_lit;
    uint32_t *d_out_len, *d_status;
} scl_lz77_sliding_replay_args;

uint64_t scl_lz77_sliding_scratch_bytes(uint64_t total_bytes, uint64_t n_streams);
int scl_lz77_sliding_parse_batch(const scl_lz77_sliding_parse_args *args, void *stream);
int scl_lz77_sliding_replay_batch(const scl_lz77_sliding_replay_args *args, void *stream);
/* the kernels that carry the index (its scatter pass), the parse and the replay, as scl_lz77_kernel_names.  The scatter
   kernel is one template on the digit source for both LZ77 coders: a trace prints the name followed by its argument. */
int scl_lz77_sliding_kernel_names(char *index, char *parse, char *replay, uint64_t cap);
/* bucket of the gram gram[0..hl): the function the kernels use, on the host.  0 for a null gram, hl outside 1..8 or m = 0 */
uint32_t scl_lz77_sliding_bucket_host(const uint8_t *gram, uint32_t hl, uint32_t m);
/* one stream in host memory, as scl_lz77_parse_host / scl_lz77_replay_host: on one wavefront below
   scl_lz77_sliding_wide_threshold() block bytes, across the whole GPU from there on (scl_lz77_sliding_*_wide below) */
int scl_lz77_sliding_parse_host(const uint8_t *h_window, uint64_t n, uint64_t start, uint32_t hash_length,
                                uint64_t hash_table_size, uint32_t max_chain_length, uint32_t lazy,
                                uint32_t min_match_length, uint32_t window_size, uint32_t *h_lit_count,
                                uint32_t *h_match_len, uint32_t *h_match_off, uint64_t seq_cap, uint64_t *n_seq,
                                uint8_t *h_literals, uint64_t lit_cap, uint64_t *n_lit);
int scl_lz77_sliding_replay_host(uint8_t *h_window, uint64_t have, uint64_t cap, uint32_t window_size,
                                 const uint32_t *h_lit_count, const uint32_t *h_match_len, const uint32_t *h_match_off,
                                 uint64_t n_seq, const uint8_t *h_literals, uint64_t n_lit, uint64_t *out_len);

/* ---- LZ77: one large stream across the whole GPU (scl_lz77_wide.hip; added to ABI 8 as above) ---------------------------
 * scl_lz77_parse_batch / scl_lz77_replay_batch give every stream one wavefront: right for thousands of streams, serial
 * for one.  These two calls take ONE stream and use the whole chip; what they store is what the batch calls store for a
 * batch of that one stream, bit for bit: sequences, literals, d_n_seq, d_n_lit, d_out_len, d_status.
 *   parse : the window is d_win[0..n), the block starts at `start` (host values: they size the launches).  The batch
 *           call's index phase is followed by: every position scored in parallel (extensions capped at `cap` bytes; a
 *           position whose match reaches the cap is LONG), per tile of `tile` positions where the chain entering at p
 *           leaves the tile, ONE wavefront walking tile to tile (it scores the LONG positions it meets in full), and one
 *           wavefront per entered tile writing rows and literals after scans over the tiles.  tile <= cap:
 *           scl_lz77_wide_shape.  d_literals is laid out like d_win: d_n_lit bytes at d_literals + start.  1 <= M <= 64
 *           only (the batch call keeps M = 0 and M > 64).  d_status: SCL_ST_CAPACITY as in the batch call.
 *   replay: appends to the slot d_win[0..cap), which holds `have` bytes: 64-bit prefix sums place every sequence, all are
 *           validated in parallel in the batch kernel's order of checks and the first fault decides d_status and
 *           d_out_len; a match byte follows root = root[root] to the history or literal byte it equals, in at most
 *           ceil(log2(n_seq + 1)) + 1 launched rounds.  Nothing outside the slot is read or written on any input.
 * Both are asynchronous on `stream` and read their scratch until they finish.  SCL_E_PARAM before any device call: a null
 * pointer, L outside 1..8, M outside 1..64, n or cap >= 2^32, start > n, have > cap, scratch misaligned (256 bytes) or
 * smaller than scl_lz77_wide_scratch_bytes(n) / scl_lz77_wide_replay_scratch_bytes(n_seq, cap - have). */
#define SCL_LZ77_WIDE_INDEX 1u
#define SCL_LZ77_WIDE_SCORE 2u /* the scores and the tile exits */
#define SCL_LZ77_WIDE_WALK 4u
#define SCL_LZ77_WIDE_EMIT 8u

typedef struct scl_lz77_wide_parse_args {
    const uint8_t *d_win;
    uint64_t n, start;
    uint32_t min_match_length, max_matches;
    uint32_t seq_cap, phases; /* phases: 0 = all, else a mask of SCL_LZ77_WIDE_* run on the same scratch, in this order
                                 (for measurements; every phase can be repeated) */
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [seq_cap] each */
    uint8_t *d_literals;                               /* n bytes */
    uint32_t *d_n_seq, *d_n_lit, *d_status;            /* one word each */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_wide_parse_args;

typedef struct scl_lz77_wide_replay_args {
    uint8_t *d_win;
    uint64_t have, cap;
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_seq] each */
    uint64_t n_seq;
    const uint8_t *d_literals;
    uint64_t n_lit;
    uint32_t *d_out_len, *d_status; /* one word each */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_wide_replay_args;

uint64_t scl_lz77_wide_scratch_bytes(uint64_t n);
uint64_t scl_lz77_wide_replay_scratch_bytes(uint64_t n_seq, uint64_t grow_bytes);
int scl_lz77_parse_wide(const scl_lz77_wide_parse_args *args, void *stream);
int scl_lz77_replay_wide(const scl_lz77_wide_replay_args *args, void *stream);
/* the compile-time shape: positions per tile and the cap of a scored extension; either may be NULL */
void scl_lz77_wide_shape(uint32_t *tile, uint32_t *cap);
/* scl_lz77_parse_host takes the wide path for a block of at least this many bytes (and 1 <= M <= 64),
   scl_lz77_replay_host for cap - have of at least this many; below it the one-wave path.  Same results either way. */
uint64_t scl_lz77_wide_threshold(void);
/* the kernels that carry the scoring, the walk and the replay's pointer doubling, as scl_lz77_kernel_names */
int scl_lz77_wide_kernel_names(char *score, char *walk, char *resolve, uint64_t cap);

/* ---- LZ77 with a sliding window: one large stream across the whole GPU (scl_lz77_sliding_wide.hip; added to ABI 8) --------
 * scl_lz77_sliding_parse_batch / scl_lz77_sliding_replay_batch give every stream one wavefront.  These two calls take ONE
 * stream and use the whole chip; what they store is what the batch calls store for a batch of that one stream, bit for
 * bit: sequences, literals, d_n_seq, d_n_lit, d_out_len, d_status.  DESIGN.md 3.6.5 has the scheme and why it is exact.
 *   parse : the window is d_win[0..n), the block starts at `start` (host values: they size the launches); the parameters
 *           are scl_lz77_sliding_parse_args'.  The sequence that starts at E is a function of E and the window alone, so
 *           the parse is the orbit of that function from `start`.  After the batch call's index phase: every
 *           candidate bit that can lead to no match under any E is cleared (the filtered bitmap); one wavefront per
 *           segment of `segment` positions follows the orbit from the segment's first position and stores every sequence
 *           in a table addressed by its E, right extensions capped at `cap` bytes and the search for a first match bounded
 *           by the end of the next segment (a sequence that reaches either is stored as OPEN and ends the segment's orbit);
 *           ONE wavefront then walks from `start`: a stored sequence is followed (a speculated one straight to its
 *           segment's exit), any other position is computed by the one-wave kernel's own code; one wavefront per segment
 *           writes rows and its own segment's literal bytes after scans over the segments.  scl_lz77_sliding_wide_shape.
 *           d_literals is laid out like d_win: d_n_lit bytes at d_literals + start.  d_status: SCL_ST_CAPACITY as in the
 *           batch call.
 *   replay: scl_lz77_replay_wide's kernels with the window's two rules: a sequence with match_length 0 copies nothing and
 *           its offset is not looked at, and an offset above min(W, bytes so far) is SCL_ST_STATE (W = 0: no bound).  Its
 *           scratch is scl_lz77_wide_replay_scratch_bytes(n_seq, cap - have).
 * Both are asynchronous on `stream` and read their scratch until they finish.  SCL_E_PARAM before any device call: a null
 * pointer, hl outside 1..8, m = 0 or m >= 2^32, C outside 1..64, mml = 0, n or cap >= 2^32, start > n, have > cap, phases
 * above 15, scratch misaligned (256 bytes) or smaller than scl_lz77_sliding_wide_scratch_bytes(n) /
 * scl_lz77_wide_replay_scratch_bytes(n_seq, cap - have). */
#define SCL_LZ77_SLIDING_WIDE_INDEX 1u
#define SCL_LZ77_SLIDING_WIDE_SPECULATE 2u
#define SCL_LZ77_SLIDING_WIDE_WALK 4u
#define SCL_LZ77_SLIDING_WIDE_EMIT 8u

typedef struct scl_lz77_sliding_wide_parse_args {
    const uint8_t *d_win;
    uint64_t n, start;
    uint64_t hash_table_size;
    uint32_t hash_length, max_chain_length;
    uint32_t lazy, min_match_length;
    uint32_t window_size, seq_cap;
    uint32_t phases, reserved; /* phases: 0 = all, else a mask of SCL_LZ77_SLIDING_WIDE_* run on the same scratch, in this
                                  order (for measurements; a walk that is repeated follows what the first one stored) */
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [seq_cap] each */
    uint8_t *d_literals;                               /* n bytes */
    uint32_t *d_n_seq, *d_n_lit, *d_status;            /* one word each */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_sliding_wide_parse_args;

typedef struct scl_lz77_sliding_wide_replay_args {
    uint8_t *d_win;
    uint64_t have, cap;
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_seq] each */
    uint64_t n_seq;
    const uint8_t *d_literals;
    uint64_t n_lit;
    uint32_t *d_out_len, *d_status; /* one word each */
    void *d_scratch;
    uint64_t scratch_bytes;
    uint32_t window_size, reserved;
} scl_lz77_sliding_wide_replay_args;

/* about 29.6 bytes per window byte: the batch call's index (12 for the sort's two permutations and its inverse, 4 for the
   keys, 0.4 for the bitmap and the histograms), 12 for the sequence table, 1 for its marks, 0.125 for the filtered bitmap,
   and 24 per segment */
uint64_t scl_lz77_sliding_wide_scratch_bytes(uint64_t n);
int scl_lz77_sliding_parse_wide(const scl_lz77_sliding_wide_parse_args *args, void *stream);
int scl_lz77_sliding_replay_wide(const scl_lz77_sliding_wide_replay_args *args, void *stream);
/* the compile-time shape: positions per segment and the cap of a speculated right extension; either may be NULL */
void scl_lz77_sliding_wide_shape(uint32_t *segment, uint32_t *cap);
/* scl_lz77_sliding_parse_host takes the wide path for a block of at least this many bytes, scl_lz77_sliding_replay_host
   for cap - have of at least this many; below it the one-wave path.  Same results either way. */
uint64_t scl_lz77_sliding_wide_threshold(void);
/* the kernels that carry the speculation, the walk and the emission, as scl_lz77_kernel_names */
int scl_lz77_sliding_wide_kernel_names(char *speculate, char *walk, char *emit, uint64_t cap);

/* ---- LZ77: the entropy stage, sequences and literals <-> block bits (scl_lz77_entropy.hip; added to ABI 8 as above) -------
 *   scl_lz77_entropy_encode_batch  <->  LZ77StreamsEncoder.encode_block   scl/compressors/lz77.py:301-361
 *   scl_lz77_entropy_decode_batch  <->  LZ77StreamsDecoder.decode_block   scl/compressors/lz77.py:364-428
 * One wavefront per stream (ONE large stream on the whole GPU: scl_lz77_entropy_*_wide below, the same bits).  A stream's
 * bits are four fields in this order: literal counts, match lengths, match offsets,
 * literals.  A sequence field is log-scale binned with o = binned_offset (0..32; the reference's default is 16): v < o is its
 * own bin, otherwise the bin is o + floor(log2(v - o + 1)) and the bits of v - o + 1 below its leading one follow as a
 * residual; the alphabet is 32 + o bins.  Each field is
 *     [32-bit counts_size][Elias-delta code of every count of the alphabet][32-bit values_size][Huffman codewords]
 * followed by its residual bits; the literals have the same shape over 256 symbols and no residuals.  A field without values
 * is one zero header, an empty stream 128 zero bits.  The Huffman code is the reference's tree over the field's own counts
 * (probabilities double(count) / double(total), Python's heapq step for step: scl_lz77_huffman_from_counts_host runs the
 * very function the kernels run).  Sequence rows, d_n_seq, d_literals / d_lit_off / d_n_lit are those of
 * scl_lz77_parse_args / scl_lz77_replay_args.
 *   encode: stream s goes to slot s of out_stride bytes (a positive multiple of 16, d_out 16-byte aligned), front to back:
 *           d_bit_off[s] = 8*s*out_stride, d_nbits[s] = its length, and every bit of the slot up to the next 32-bit word
 *           boundary behind the stream is defined.  All sizes are known before a bit is stored, so a stream with a non-zero
 *           status stores NOTHING: SCL_ST_CAPACITY = the slot is too small (d_nbits[s] still reports the length needed) or
 *           the stream has 2^32 bits or more (d_nbits[s] = 2^32 - 1); SCL_ST_SIZE = a codeword longer than 32 bits (a field
 *           of at least 14 930 351 values with Fibonacci counts), d_n_seq[s] > seq_cap or a literal range outside
 *           lit_bytes; SCL_ST_SYMBOL = a value without a bin (binned_offset 0 and the value 2^32 - 1: the reference raises
 *           "too large").  d_nbits[s] = 0 for the last two.
 *   decode: stream s is the d_in_nbits[s] bits from absolute bit d_bit_off[s] of d_in, at any alignment; bits behind the
 *           block are not an error.  The values go to row s (seq_cap entries) of the three arrays and to the literal range
 *           [d_lit_off[s], d_lit_off[s] + d_lit_cap[s]) of d_literals; d_n_seq[s] = the count of the shortest sequence
 *           field, d_n_lit[s] = the literals, d_consumed[s] = LZ77StreamsDecoder.decode_block's num_bits_consumed.  The
 *           stream stops at its first fault, and what its rows (up to seq_cap entries) and its literal range then hold is
 *           undefined -- a field may be left half turned from bins into values; d_n_seq[s] counts whole sequences of
 *           the fields decoded before the fault, 0 unless all three were.  SCL_ST_TRUNCATED = a header or a section reaches past d_in_nbits[s];
 *           SCL_ST_STATE = the counts section is not used up exactly, holds fewer counts than the alphabet (more are
 *           ignored), only zeros, or a count of 2^32 or more; a codeword cut by the end of its section or a bit into the
 *           missing child of the one-symbol code; a value that no 32-bit field holds; field counts that differ;
 *           SCL_ST_CAPACITY = more values than a row or a literal range holds (nothing is stored past it); SCL_ST_SIZE = a
 *           code above 32 bits, or an input or literal range outside its buffer.
 * Nothing outside a stream's own slot / input bits / rows / literal range is read or written on any input; no kernel uses
 * device scratch.  Both calls are asynchronous on `stream`.  SCL_E_PARAM before any device call: a null pointer,
 * binned_offset above 32, n_streams >= 2^32, a bad out_stride or a misaligned d_out. */
typedef struct scl_lz77_entropy_encode_args {
    uint64_t n_streams;
    uint32_t seq_cap, binned_offset;
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    const uint32_t *d_n_seq;
    const uint8_t *d_literals;
    uint64_t lit_bytes;
    const uint64_t *d_lit_off; /* [n_streams] */
    const uint32_t *d_n_lit;
    uint8_t *d_out;            /* [n_streams * out_stride] */
    uint64_t out_stride;
    uint64_t *d_bit_off;       /* [n_streams] each */
    uint32_t *d_nbits, *d_status;
} scl_lz77_entropy_encode_args;

typedef struct scl_lz77_entropy_decode_args {
    const uint8_t *d_in;
    uint64_t in_size_bytes;
    const uint64_t *d_bit_off; /* [n_streams] */
    const uint32_t *d_in_nbits;
    uint64_t n_streams;
    uint32_t seq_cap, binned_offset;
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_streams * seq_cap] each */
    uint32_t *d_n_seq;
    uint8_t *d_literals;
    uint64_t lit_bytes;
    const uint64_t *d_lit_off; /* [n_streams] */
    const uint32_t *d_lit_cap;
    uint32_t *d_n_lit, *d_consumed, *d_status;
} scl_lz77_entropy_decode_args;

int scl_lz77_entropy_encode_batch(const scl_lz77_entropy_encode_args *args, void *stream);
int scl_lz77_entropy_decode_batch(const scl_lz77_entropy_decode_args *args, void *stream);
/* a multiple of 128 that holds any stream of at most max_n_seq sequences and max_n_lit literals: the headers, the counts
   at 43 bits each, 31 residual bits per sequence value, and for the codewords of a field of n values n * (ceil(log2 K) + 1)
   bits IN TOTAL.  That is a bound on the field, not on a codeword (one codeword may have 32 bits): a Huffman code of the
   values' own counts spends less than n * (H + 1) bits on them, H their empirical entropy, and H <= log2 K. */
uint64_t scl_lz77_entropy_slot_bytes(uint64_t max_n_seq, uint64_t max_n_lit, uint32_t binned_offset);
/* as scl_lz77_kernel_names */
int scl_lz77_entropy_kernel_names(char *enc, char *dec, uint64_t cap);
/* The tree builder of the two kernels, on the host (no device): code[i] / len[i] = the codeword of symbol i, most
   significant bit first in the low len[i] bits, 0 / 0 for a symbol without a count.  SCL_E_PARAM: K outside 1..256, a count
   of 2^32 or more, no count at all, a codeword longer than 32 bits. */
int scl_lz77_huffman_from_counts_host(const uint64_t *counts, uint32_t K, uint32_t *code, uint8_t *len);

/* ---- LZ77: the entropy stage of ONE large stream across the whole GPU (scl_lz77_entropy_wide.hip; added to ABI 8 as above)
 * scl_lz77_entropy_*_batch give every stream one wavefront -- and the decoder's walk one lane.  These two calls take ONE
 * stream and use the whole chip; the bits, the rows, the literals, n_seq / n_lit / consumed and the status are what the
 * batch calls give for a batch of that one stream (the layout and the status rules above), with two differences that the
 * 32-bit words of the batch calls cannot express: d_nbits and `consumed` are 64-bit, and a stream of 2^32 bits or more is
 * coded as long as every section fits its own 32-bit header (SCL_ST_CAPACITY otherwise, d_nbits = the length needed).
 *   encode: the first n_seq entries of the three rows and n_lit literals from d_literals[0] on (host values: they size the
 *           launches) -> d_out[0 .. out_cap_bytes), front to back.  Grid-wide histograms, ONE workgroup for the four trees
 *           and the 64-bit position of every header and section, then every section emitted in tiles of 4096 values at its
 *           own bit position.  All faults are decided before a bit is stored: a stream with a non-zero *d_status stores
 *           NOTHING, no byte at or past d_out + out_cap_bytes is ever written, and *d_nbits is the length needed also for
 *           SCL_ST_CAPACITY (0 for SCL_ST_SIZE / SCL_ST_SYMBOL).  Asynchronous on `stream`, no host read-back.
 *   decode: the in_nbits bits from bit in_bit_offset of d_in (any bit alignment; d_in itself 4-byte aligned) -> the first
 *           entries of the three rows (seq_cap each) and of d_literals (lit_cap bytes), and *d_result.  Field by field -- a
 *           field's position is known only when the one before it is decoded: one workgroup reads the headers and counts
 *           and builds the tree and a lookup table in scratch, the codewords are decoded by the self-synchronising scheme of
 *           scl_prefix_decode_block (128 bits per thread, 256 threads per workgroup, passes relaunched until no workgroup's
 *           exit moves; result.sync_passes = the passes, summed over the fields, in which a workgroup moved its start),
 *           and the bins become values grid-wide after a 64-bit scan of the residual widths.  First fault wins, in field
 *           order, with the batch decoder's status for the same damage.
 *           SYNCHRONISING: the call reads device words between passes and between fields and returns when everything but
 *           the last field's kernels has finished; per field it synchronises once for the headers and once per pass, at
 *           most 1 + (workgroups of the field - 1) times, 4 + sum over the fields in all.
 * No kernel waits on another workgroup (no flags, no look-back, no cooperative launch); nothing outside the output bytes,
 * the input bytes d_in[0 .. in_size_bytes), the rows up to n_seq / seq_cap and the literal range is read or written on any
 * input.  SCL_E_PARAM before any device call, the message prefixed with the entry point's name: a null pointer,
 * binned_offset above 32, n_seq / n_lit / seq_cap / lit_cap of 2^32 or more, in_nbits of 2^46 or more, a stream that ends
 * behind in_size_bytes, d_out / d_in not 4-byte or rows not 4-byte or d_scratch / d_nbits / d_result not 8-byte aligned,
 * scratch smaller than scl_lz77_entropy_wide_scratch_bytes. */
typedef struct scl_lz77_entropy_wide_encode_args {
    const uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [n_seq] each */
    uint64_t n_seq;
    const uint8_t *d_literals;
    uint64_t n_lit;
    uint32_t binned_offset, reserved;
    uint8_t *d_out;
    uint64_t out_cap_bytes;
    uint64_t *d_nbits;  /* one u64 */
    uint32_t *d_status; /* one word */
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_entropy_wide_encode_args;

typedef struct scl_lz77_entropy_wide_result {
    uint64_t consumed;
    uint32_t n_seq, n_lit, status, sync_passes;
} scl_lz77_entropy_wide_result;

typedef struct scl_lz77_entropy_wide_decode_args {
    const uint8_t *d_in;
    uint64_t in_size_bytes, in_bit_offset, in_nbits;
    uint32_t binned_offset, reserved;
    uint64_t seq_cap, lit_cap;
    uint32_t *d_lit_count, *d_match_len, *d_match_off; /* [seq_cap] each */
    uint8_t *d_literals;                               /* lit_cap bytes */
    scl_lz77_entropy_wide_result *d_result;
    void *d_scratch;
    uint64_t scratch_bytes;
} scl_lz77_entropy_wide_decode_args;

int scl_lz77_entropy_encode_wide(const scl_lz77_entropy_wide_encode_args *args, void *stream);
int scl_lz77_entropy_decode_wide(const scl_lz77_entropy_wide_decode_args *args, void *stream);
/* scratch for either call: encode of n_seq sequences and n_lit literals, decode with seq_cap = n_seq, lit_cap = n_lit and
   in_nbits; monotone in every argument */
uint64_t scl_lz77_entropy_wide_scratch_bytes(uint64_t n_seq, uint64_t n_lit, uint64_t in_nbits);
/* The stream size from which both wide calls beat the one-wave kernels, counted in CODED VALUES, 3 * n_seq + n_lit: the
   smallest measured stream from which both wide calls won at every larger measured stream on both sources (DESIGN.md
   3.6.3).  Values, not block bytes: 16 MiB of equal bytes parse to 1 sequence and 6 literals, and on those 9 values one
   wavefront is 0.03 ms ahead of the wide call's launches.  Below it scl_lz77_entropy_*_batch on a batch of one is the
   faster route to the same bits; nothing in the library routes by it. */
uint64_t scl_lz77_entropy_wide_threshold(void);
/* the kernels that carry the emission, the decoder's synchronisation and the residuals, as scl_lz77_kernel_names */
int scl_lz77_entropy_wide_kernel_names(char *emit, char *sync, char *resid, uint64_t cap);

/* ---- stream compaction / framing ------------------------------------------------------------ */
#define SCL_COMPACT_DENSE 0  /* stream c left-aligned at byte d_out_byte_offset[c], zero tail   */
#define SCL_COMPACT_FRAMED 1 /* EncodedBlockWriter framing per stream:
                                [u32 BE payload bytes][3-bit pad count][pad zeros][stream bits]
                                (encoded_stream.py:23-46,94-103,150-175)                         */

/* Gathers n_chunks streams (d_bit_offset, d_nbits) of d_in into one dense buffer.
   d_out_byte_offset has n_chunks+1 entries (exclusive prefix sum of the per-stream byte sizes;
   the last entry is the total).  d_scratch must hold scl_streams_compact_scratch_bytes(n_chunks).
   Fails per call (not per chunk): if the total exceeds out_capacity nothing past it is written
   and d_out_byte_offset[n_chunks] still reports the required size. */
uint64_t scl_streams_compact_scratch_bytes(uint64_t n_chunks);
int scl_streams_compact(const uint8_t *d_in, const uint64_t *d_bit_offset, const uint32_t *d_nbits,
                        uint64_t n_chunks, int mode, uint8_t *d_out, uint64_t out_capacity,
                        uint64_t *d_out_byte_offset, void *d_scratch, void *stream);
/* (ABI version 5) the same with the first record at byte *d_base of d_out, d_base in DEVICE memory (NULL = 0); the offsets
   written are absolute (entry 0 = *d_base, entry n = where the next record would start).  Sub-batch i + 1 of a batch passes
   the address of sub-batch i's last offset entry (it may be the address its own entry 0 goes to): one dense buffer and one
   offset table without the host ever learning a size -- so that a sub-batch can be compacted on a second stream while the
   next one is still being encoded. */
int scl_streams_compact_at(const uint8_t *d_in, const uint64_t *d_bit_offset, const uint32_t *d_nbits,
                           uint64_t n_chunks, int mode, uint8_t *d_out, uint64_t out_capacity,
                           uint64_t *d_out_byte_offset, const uint64_t *d_base, void *d_scratch, void *stream);

/* ---- wave-striped slots (ABI version 8) --------------------------------------------------------------------------------
 * A second MEMORY layout for the slots of a batch, written and read by the tuned rANS kernels (and by the tANS models
 * those kernels serve).  Nothing changes logically: stream c is still nbits[c] bits at bit offset bit_offset[c] =
 * 8*(c+1)*out_stride - nbits[c] of a buffer of slots of out_stride bytes -- rANSEncoder.encode_block's bits
 * (scl/compressors/rANS.py:186-210), in the positions the plain entry points put them -- but the 64 slots of a wavefront
 * are interleaved in 16-byte pieces:
 *     logical byte A = c*out_stride + b   lives at   (c/64)*64*out_stride + (b/16)*1024 + 16*(c%64) + b%16
 * so that piece q of the 64 lanes of a wave is one contiguous kilobyte.  A lane then stores 16 bytes at a time where the
 * linear layout made it buffer whole 128-byte lines (256 B of LDS per lane: two waves per SIMD); the striped encoder runs
 * four waves per SIMD and stores row by row, 64 adjacent pieces per instruction.  d_out must hold
 * round_up(n_chunks, 64) * out_stride bytes.  Worth it for batches that fill the chip (>= ~196 608 chunks on MI355X:
 * 1 GiB headline batch encode 0.55 -> 0.52 ms); smaller batches are faster on the linear entry points.
 *   scl_*_striped_ok              1 if the striped entry points serve this model (= the tuned kernels do: fast_path with
 *                                 NUM_BITS_OUT = 1 or in {4, 8, 16}, alphabet <= 256), else 0 -- they then fail with
 *                                 SCL_E_PARAM, as they do while the calling thread keeps the tuned kernels out;
 *   scl_*_encode_batch_striped    arguments of scl_rans_encode_batch; out_stride < 2^24 and, for rANS / tANS,
 *                                 >= scl_*_slot_bytes(chunk_len) (the range coder takes shorter slots: a stream that
 *                                 does not fit gets SCL_ST_CAPACITY, as on linear slots);
 *   scl_*_decode_batch_striped    arguments of scl_rans_decode_batch with in_stride (the encoder's out_stride) in place of
 *                                 in_size_bytes; stream c must lie inside logical slot c;
 *   scl_streams_compact_striped   scl_streams_compact_at on striped slots: the SAME dense / framed bytes as the linear
 *                                 path produces (BitArray.tobytes() of every block back to back, or the reference's file
 *                                 format, encoded_stream.py:150-175) -- the only form the reference ever sees;
 *   scl_*_kernel_names_striped    scl_*_kernel_names for the striped kernels. */
int scl_rans_striped_ok(const scl_rans_model *m);
int scl_tans_striped_ok(const scl_tans_model *m);
/* the range coder (RangeEncoder.encode_block / RangeDecoder.decode_block, range_coder.py:188-207, :269-317) on the same
   layout: streams grow front to back, bit_offset[c] = 8*c*out_stride as on linear slots; served: PRECISION = 32 models over
   uniform bytes (configs[2]) and over tables with totals 256..4096 (what the cooperative line store of the linear kernels
   cannot help: lanes that are not in lockstep) */
int scl_range_striped_ok(const scl_range_model *m);
int scl_range_encode_batch_striped(const scl_range_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                                   const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                   uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                   uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_range_decode_batch_striped(const scl_range_model *m, const uint8_t *d_in, uint64_t in_stride,
                                   const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                   uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                                   uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                   uint32_t *d_status, void *stream);
int scl_rans_kernel_names_striped(const scl_rans_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
int scl_tans_kernel_names_striped(const scl_tans_model *m, uint64_t n_chunks, char *enc, char *dec, uint64_t cap);
int scl_rans_encode_batch_striped(const scl_rans_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                                  const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                  uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                  uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_rans_decode_batch_striped(const scl_rans_model *m, const uint8_t *d_in, uint64_t in_stride,
                                  const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                  uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                                  uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                  uint32_t *d_status, void *stream);
int scl_tans_encode_batch_striped(const scl_tans_model *m, const uint8_t *d_sym, uint64_t sym_stride,
                                  const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                  uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                  uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_tans_decode_batch_striped(const scl_tans_model *m, const uint8_t *d_in, uint64_t in_stride,
                                  const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                  uint64_t n_chunks, uint8_t *d_out_sym, uint64_t out_stride,
                                  uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                  uint32_t *d_status, void *stream);
int scl_streams_compact_striped(const uint8_t *d_in, uint64_t in_stride, const uint64_t *d_bit_offset,
                                const uint32_t *d_nbits, uint64_t n_chunks, int mode, uint8_t *d_out,
                                uint64_t out_capacity, uint64_t *d_out_byte_offset, const uint64_t *d_base,
                                void *d_scratch, void *stream);

/* (ABI version 7) Host-side index of a framed block file held in host memory -- the walk EncodedBlockReader.get_block makes
   one record at a time (encoded_stream.py:196-225) followed by Padder.remove_byte_padding (:48-58), for a whole buffer:
   for every COMPLETE record [u32 BE payload bytes][payload] starting at h_buf[0] writes where its stream starts (bit offset
   from h_buf), its number of stream bits and the value of its first size_bits bits (the block's DATA_BLOCK_SIZE_BITS
   header; size_bits <= 64).  Stops in front of the first record that crosses buf_size or after max_records; *n_records
   = records indexed, *consumed = bytes they span (what is left belongs to the next buffer -- or is a truncated file).
   No device, no stream.  SCL_E_PARAM (with *n_records / *consumed = what came before) for a record with an empty payload
   or one shorter than its padding and size header. */
int scl_framed_index_host(const uint8_t *h_buf, uint64_t buf_size, uint32_t size_bits, uint64_t max_records,
                          uint64_t *h_bit_offset, uint64_t *h_nbits, uint64_t *h_block_size,
                          uint64_t *n_records, uint64_t *consumed);

/* ---- multi-GPU: variable-length gather of compacted streams over RCCL (SURVEY.md 8e, configs[4]) ------
 * No reference counterpart (the reference has no communication).  One process per GPU; every rank encodes and
 * compacts its own block-contiguous shard, then the dense payloads go to one rank: an all-gather of the byte
 * counts, then one grouped ncclSend / ncclRecv per sender straight into the root's buffer at the prefix offsets
 * (xGMI is point to point: the root receives on all its links at once).  RCCL is dlopen'ed on first use.
 *   scl_rccl_unique_id      : rank 0 creates the 128-byte id and hands it to the others out of band (any channel);
 *   scl_rccl_comm_create    : collective over the `world` ranks; the communicator belongs to the current device;
 *   scl_rccl_allgather_u64  : collective; one u64 per rank -> h_out[world] on every rank (synchronises `stream`):
 *                             the byte counts, so that the root can size its buffer before anything is posted;
 *   scl_rccl_allgather_async: collective, asynchronous on `stream`, device to device: n_u64 values per rank ->
 *                             d_out[world * n_u64] on every rank; nothing waits for the host (the overlapped
 *                             pipeline queues it behind a sub-batch's compaction and reads it back with an event);
 *   scl_streams_gather_rccl : collective, asynchronous on `stream`: rank r's send_bytes bytes arrive at the root's
 *                             d_recv + h_rank_offsets[r]; h_rank_offsets[world + 1] (host) = exclusive prefix sum
 *                             of the counts, last entry = total.  d_recv matters on the root only;
 *   scl_streams_gatherv_rccl: n_parts such gathers (a payload and its per-chunk offset table, say) in ONE grouped
 *                             exchange: part p moves h_send_bytes[p] bytes from d_send[p] to the root's d_recv[p]
 *                             + h_rank_offsets[p * (world + 1) + r].
 *   scl_streams_gather_blocks_rccl: configs[4]'s exchange as one call: a (sub-)batch's dense payload and its
 *                             n_chunks + 1 record offsets go to the root in one grouped exchange, and the root shifts
 *                             every rank's offsets by the bytes of the ranks before it (one small kernel on `stream`),
 *                             so d_recv_offsets [sum chunks + 1] is the offset table a single process would have
 *                             produced; h_bytes_by_rank / h_chunks_by_rank [world] are the exchanged counts.
 *   Errors: all arguments are checked before anything is posted; after ncclGroupStart the group is closed on every
 *   path (first error recorded, ncclGroupEnd, then return).  A layout that contradicts this rank's own count is
 *   refused on this rank only -- the peers then wait in the exchange, so derive layouts from exchanged counts. */
/*   scl_rccl_comm_info      : (ABI version 5) what the communicator reports about itself -- ncclCommUserRank /
 *                             ncclCommCount -- and the device it belongs to;
 *   scl_rccl_inject_api     : (ABI version 5) TEST HOOK.  Every RCCL operation above goes through one table of eleven
 *                             plain-C function pointers (scl_rccl_api); by default it is filled from librccl.so on first
 *                             use, this call replaces it (NULL restores the default).  With host_memory != 0 the
 *                             buffers handed to the calls above are host memory and the library makes no HIP call on
 *                             these paths (its own copies are memcpy, the root's offset fix-up a loop): the tests run a
 *                             W-rank exchange -- layout checks, grouped posts, the root's receive offsets -- inside one
 *                             process on a machine without a GPU.  Not for production use. */
typedef struct scl_comm scl_comm;
typedef struct scl_rccl_api {
    int (*get_unique_id)(uint8_t *id128);                                       /* ncclGetUniqueId    */
    int (*comm_init_rank)(void **comm, int nranks, const uint8_t *id128, int rank); /* ncclCommInitRank */
    int (*comm_destroy)(void *comm);                                            /* ncclCommDestroy    */
    int (*comm_count)(void *comm, int *nranks);                                 /* ncclCommCount      */
    int (*comm_user_rank)(void *comm, int *rank);                               /* ncclCommUserRank   */
    int (*all_gather)(const void *send, void *recv, uint64_t count, int dtype, void *comm, void *stream);
    int (*send)(const void *buf, uint64_t count, int dtype, int peer, void *comm, void *stream);
    int (*recv)(void *buf, uint64_t count, int dtype, int peer, void *comm, void *stream);
    int (*group_start)(void);
    int (*group_end)(void);
    const char *(*error_string)(int result);
    int host_memory; /* 1: buffers are host memory, the library makes no HIP call around the exchange */
} scl_rccl_api;      /* dtype: 1 = uint8, 5 = uint64 (ncclDataType_t); results: 0 = success */
int scl_rccl_inject_api(const scl_rccl_api *api);
int scl_rccl_comm_info(scl_comm *c, int *rank, int *nranks, int *device);
int scl_rccl_unique_id(uint8_t *id128);
int scl_rccl_comm_create(const uint8_t *id128, int rank, int world, scl_comm **out);
void scl_rccl_comm_destroy(scl_comm *c);
int scl_rccl_allgather_u64(scl_comm *c, uint64_t value, uint64_t *h_out, void *stream);
int scl_rccl_allgather_async(scl_comm *c, const uint64_t *d_in, uint64_t *d_out, uint64_t n_u64, void *stream);
int scl_streams_gather_rccl(scl_comm *c, int root, const uint8_t *d_send, uint64_t send_bytes, uint8_t *d_recv,
                            const uint64_t *h_rank_offsets, void *stream);
int scl_streams_gatherv_rccl(scl_comm *c, int root, uint32_t n_parts, const uint8_t *const *d_send,
                             const uint64_t *h_send_bytes, uint8_t *const *d_recv, const uint64_t *h_rank_offsets,
                             void *stream);
int scl_streams_gather_blocks_rccl(scl_comm *c, int root, const uint8_t *d_payload, uint64_t payload_bytes,
                                   const uint64_t *d_offsets, uint64_t n_chunks, uint8_t *d_recv_payload,
                                   uint64_t *d_recv_offsets, const uint64_t *h_bytes_by_rank,
                                   const uint64_t *h_chunks_by_rank, void *stream);

/* ---- model construction helper (row f3): symbol histogram ------------------------------------------ */
/* d_counts[256] (uint64) += number of occurrences of every byte value in d_sym[0..n).  The caller zeroes
   d_counts.  Equals DataBlock.get_counts() (scl/core/data_block.py:37-62) for uint8 data. */
int scl_histogram_u8(const uint8_t *d_sym, uint64_t n, uint64_t *d_counts, void *stream);
/* the same for uint16 symbol indices of an alphabet of K <= 65536 symbols: d_counts[K] += occurrences; indices >= K are
   not counted but tallied in *d_out_of_range (uint32, zeroed by the caller).  ABI 4. */
int scl_histogram_u16(const uint16_t *d_sym, uint64_t n, uint32_t K, uint64_t *d_counts,
                      uint32_t *d_out_of_range, void *stream);

/* ---- host convenience (one chunk, host buffers; allocates, copies, runs N=1, synchronises) --- */
/* These back the drop-in encode_block / decode_block of the Python classes.  h_out receives the
   left-aligned stream (what BitArray.tobytes() would give); *nbits its length. */
int scl_rans_encode_host(const scl_rans_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                         uint64_t out_cap_bytes, uint64_t *nbits);
int scl_rans_decode_host(const scl_rans_model *m, const uint8_t *h_in, uint64_t in_nbits,
                         uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_tans_encode_host(const scl_tans_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                         uint64_t out_cap_bytes, uint64_t *nbits);
int scl_tans_decode_host(const scl_tans_model *m, const uint8_t *h_in, uint64_t in_nbits,
                         uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_range_encode_host(const scl_range_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                          uint64_t out_cap_bytes, uint64_t *nbits);
int scl_range_decode_host(const scl_range_model *m, const uint8_t *h_in, uint64_t in_nbits,
                          uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_aec_encode_host(const scl_aec_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                        uint64_t out_cap_bytes, uint64_t *nbits);
int scl_aec_decode_host(const scl_aec_model *m, const uint8_t *h_in, uint64_t in_nbits,
                        uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
/* one block of a coder whose state the caller keeps on the host between calls (h_counts / h_past_k are
   read before and rewritten after the block): ArithmeticEncoder.encode_block / ArithmeticDecoder.decode_block
   on an object that has coded blocks before (arithmetic_coding.py:52-56) */
int scl_aec_encode_host_resume(const scl_aec_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                               uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *h_counts,
                               uint32_t *h_past_k);
int scl_aec_decode_host_resume(const scl_aec_model *m, const uint8_t *h_in, uint64_t in_nbits,
                               uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                               uint32_t *h_counts, uint32_t *h_past_k);
/* peek the DATA_BLOCK_SIZE_BITS header of a host stream (so callers can size h_out_sym) */
int scl_stream_block_size_host(const uint8_t *h_in, uint64_t in_nbits, uint32_t size_bits,
                               uint64_t *n_out);

/* ---- alphabets of up to 65536 symbols: uint16 symbol indices (ABI 4) ---------------------------------
 * The reference codes any hashable alphabet (Frequencies.freq_dict, prob_dist.py:193-205); its LZ77 / text models
 * reach past 256 symbols.  Every batch / host entry point above has a *_u16 twin with the same arguments, the
 * symbol arrays typed uint16_t and the symbol strides counted in SYMBOLS.  They take ANY model handle (models of
 * more than 256 symbols are refused by the uint8 entry points with SCL_E_PARAM) and run the any-parameter kernels:
 * tables are read where they are in device memory, adaptive order-k / i.i.d. rows are scanned linearly (cost per
 * symbol grows with the alphabet).  For a model of at most 256 symbols the stream equals the uint8 entry point's. */
int scl_rans_encode_batch_u16(const scl_rans_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                              const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                              uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                              uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_rans_decode_batch_u16(const scl_rans_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                              const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                              uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                              uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                              uint32_t *d_status, void *stream);
int scl_tans_encode_batch_u16(const scl_tans_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                              const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                              uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                              uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_tans_decode_batch_u16(const scl_tans_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                              const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                              uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                              uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                              uint32_t *d_status, void *stream);
int scl_range_encode_batch_u16(const scl_range_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                               const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                               uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                               uint32_t *d_out_nbits, uint32_t *d_status, void *stream);
int scl_range_decode_batch_u16(const scl_range_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                               const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                               uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                               uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                               uint32_t *d_status, void *stream);
int scl_aec_encode_batch_u16(const scl_aec_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                             const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                             uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                             uint32_t *d_out_nbits, uint32_t *d_status, void *d_scratch,
                             uint64_t scratch_bytes, void *stream);
int scl_aec_decode_batch_u16(const scl_aec_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                             const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                             uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                             uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                             uint32_t *d_status, void *d_scratch, uint64_t scratch_bytes,
                             void *stream);
int scl_aec_encode_batch_resume_u16(const scl_aec_model *m, const uint16_t *d_sym, uint64_t sym_stride,
                                    const uint32_t *d_lens, uint32_t chunk_len, uint64_t n_chunks,
                                    uint8_t *d_out, uint64_t out_stride, uint64_t *d_out_bit_offset,
                                    uint32_t *d_out_nbits, uint32_t *d_status, void *d_state,
                                    uint64_t state_bytes, uint64_t n_coders, void *stream);
int scl_aec_decode_batch_resume_u16(const scl_aec_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                    const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,
                                    uint64_t n_chunks, uint16_t *d_out_sym, uint64_t out_stride,
                                    uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed,
                                    uint32_t *d_status, void *d_state, uint64_t state_bytes, uint64_t n_coders,
                                    void *stream);
int scl_rans_encode_host_u16(const scl_rans_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                             uint64_t out_cap_bytes, uint64_t *nbits);
int scl_rans_decode_host_u16(const scl_rans_model *m, const uint8_t *h_in, uint64_t in_nbits,
                             uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_tans_encode_host_u16(const scl_tans_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                             uint64_t out_cap_bytes, uint64_t *nbits);
int scl_tans_decode_host_u16(const scl_tans_model *m, const uint8_t *h_in, uint64_t in_nbits,
                             uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_range_encode_host_u16(const scl_range_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                              uint64_t out_cap_bytes, uint64_t *nbits);
int scl_range_decode_host_u16(const scl_range_model *m, const uint8_t *h_in, uint64_t in_nbits,
                              uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_aec_encode_host_u16(const scl_aec_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                            uint64_t out_cap_bytes, uint64_t *nbits);
int scl_aec_decode_host_u16(const scl_aec_model *m, const uint8_t *h_in, uint64_t in_nbits,
                            uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed);
int scl_aec_encode_host_resume_u16(const scl_aec_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                                   uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *h_counts,
                                   uint32_t *h_past_k);
int scl_aec_decode_host_resume_u16(const scl_aec_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                   uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                                   uint32_t *h_counts, uint32_t *h_past_k);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_H */
