// scl_fixed.hip -- batched fixed-width coding of symbol indices for gfx950: a stream across as many workgroups as it has tiles.
//
// The data section of the reference's FixedBitwidthEncoder: index i of a stream of width w is the w stream bits
// [i * w, (i + 1) * w), MSB first.  No table, no state, no scan, no second pass: where a symbol lands follows from its index.
// 32 symbols of width w are exactly w 32-bit words for every w, so
//   a lane's group   = 32 symbols            = w words,
//   a workgroup's tile = 256 groups = SCL_FIXED_TILE symbols = 256 * w words = 64 * w pieces of 16 bytes,
// and no two lanes, let alone two workgroups, share an output word: no atomics on the data path, no order between workgroups.
// Grid = (tiles of the longest stream) x (streams); a workgroup past its stream's end leaves at once.  The same pair is
// therefore the lane-parallel batch path AND the whole-GPU path of one large stream.
//
// Data movement, both kernels: global <-> LDS in 16-byte pieces, adjacent lanes on adjacent pieces; a lane packs or unpacks
// its group between registers and LDS words (the width is uniform per workgroup and lives in scalar registers).  One LDS
// buffer serves the way in and the way out (barriers in between): 8 KiB for byte rows up to 32 KiB + 64 B at w = 32.
//   encode: symbol pieces -> LDS; lane: 32 symbols -> w big-endian words at LDS word tid * w; LDS -> slot pieces.
//           The last, partial piece of a row is read symbol by symbol, the last, partial piece of a stream is stored word
//           by word: nothing is read at or past symbol n, nothing stored past the stream's last word or the slot's end.
//   decode: the tile's bit window starts at ANY bit: the pieces that hold it -> LDS (a piece that crosses in_size_bytes byte by
//           byte, nothing at or past in_size_bytes), the window's start within its first piece is a shift the lanes carry;
//           lane: a sequential reader over w + 2 LDS words -> 32 symbols -> LDS; LDS -> row pieces, the last partial piece
//           symbol by symbol.
// Statuses: the call zeroes d_status; lane 0 of a stream's first workgroup raises what follows from the stream's numbers
// alone (CAPACITY, TRUNCATED), any lane that meets an index >= K raises SYMBOL, with an atomic OR on the fault path only.
// include/scl_hip.h has the contract, DESIGN.md 3.5.4 the measurements.
#include <vector>

#include "scl_entry.h"

#define FX_THREADS 256u
#define FX_GROUP 32u
#define FX_TILE (FX_THREADS * FX_GROUP)
static_assert(FX_TILE == SCL_FIXED_TILE, "the header names the tile");
// The LDS of a workgroup, sized by the launch for the widest stream of the batch (narrow streams leave room for more
// workgroups a CU): a tile of symbols on one side, on the other the tile's 64 * w pieces -- for the decoder one more for the
// bit offset and the reader's look-ahead: a lane's first word is at most (127 + 255 * 32 * w) / 32, it reads two words there
// and at most w + 1 behind them, so no word at or past 256 * w + 7 = piece 64 * w + 2.
template <class SYM>
static u32 fx_lds_bytes(u32 w_max) {
    const u32 symbols = FX_TILE * (u32)sizeof(SYM), stream = (64u * w_max + 4u) * 16u;
    return symbols > stream ? symbols : stream;
}

struct FxParams {
    const u64 *wk;  // per stream: K in the low 40 bits, the width above; null: every stream has `same`
    u64 same;
    u32 tiles;  // workgroups a stream: tiles of the longest one
};

template <class SYM>
struct FxRow {
    static constexpr u32 E = 16 / sizeof(SYM);              // symbols a piece
    static constexpr u32 PIECES = FX_TILE / E;              // pieces a full tile of symbols
    static constexpr u32 WORDS = FX_GROUP * sizeof(SYM) / 4;  // words a lane's group of symbols
};

// symbol i (a constant after unrolling) of a lane's group held as words
template <class SYM>
__device__ __forceinline__ u32 fx_get(const u32 *q, u32 i) {
    if constexpr (sizeof(SYM) == 1) return (q[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    else if constexpr (sizeof(SYM) == 2) return (q[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    else return q[i];
}
template <class SYM>
__device__ __forceinline__ void fx_set(u32 *q, u32 i, u32 s) {
    if constexpr (sizeof(SYM) == 1) q[i >> 2] |= s << (8 * (i & 3));
    else if constexpr (sizeof(SYM) == 2) q[i >> 1] |= s << (16 * (i & 1));
    else q[i] = s;
}

// A lane's group of 32 symbols (words q) -> w big-endian words at wout.  MASK: the tile is not full, symbols at and past
// `cnt` are not symbols (pieces past the row's end were never staged).  -> an index above kmax was met (coded as 0).
// w is uniform and the loop unrolled: how many bits are pending after symbol i is scalar arithmetic.
template <class SYM, bool MASK>
__device__ __forceinline__ bool fx_pack_group(const u32 *q, u32 g0, u32 cnt, u32 w, u32 kmax, u32 *wout) {
    u64 acc = 0;
    u32 have = 0, k = 0;
    bool bad = false;
#pragma unroll
    for (u32 i = 0; i < FX_GROUP; ++i) {
        u32 s = fx_get<SYM>(q, i);
        if (MASK && g0 + i >= cnt) s = 0;
        if (s > kmax) {
            bad = true;
            s = 0;
        }
        acc = (acc << w) | s;
        have += w;
        if (have >= 32) {
            have -= 32;
            wout[k++] = scl_bswap32((u32)(acc >> have));
        }
    }
    return bad;
}

// The 32 symbols of a lane's group out of the LDS words lw, from window bit `pos` on: a sequential reader over w + 2 words.
template <class SYM, bool MASK>
__device__ __forceinline__ bool fx_unpack_group(const u32 *lw, u32 pos, u32 g0, u32 cnt, u32 w, u32 kmax, u32 *q) {
    u32 idx = pos >> 5;
    const u32 s0 = pos & 31;
    u64 acc = (((u64)scl_bswap32(lw[idx]) << 32) | scl_bswap32(lw[idx + 1])) << s0;
    u32 have = 64 - s0;  // valid bits at the top of acc; >= 32 before every symbol
    idx += 2;
    bool bad = false;
#pragma unroll
    for (u32 i = 0; i < FX_GROUP; ++i) {
        u32 s = (u32)(acc >> (64 - w));
        acc <<= w;
        have -= w;
        if (have < 32) {
            acc |= (u64)scl_bswap32(lw[idx++]) << (32 - have);
            have += 32;
        }
        if (MASK && g0 + i >= cnt) s = 0;  // (bits behind the stream's last symbol)
        if (s > kmax) {
            bad = true;
            s = 0;
        }
        fx_set<SYM>(q, i, s);
    }
    return bad;
}

template <class SYM>
__global__ void __launch_bounds__(FX_THREADS, 4)
    fixed_encode_kernel(FxParams P, const SYM *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens, u32 chunk_len,
                        u64 n_chunks, u8 *__restrict__ out, u64 out_stride, u64 *__restrict__ out_bit_off,
                        u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    using R = FxRow<SYM>;
    extern __shared__ __attribute__((aligned(16))) uint4 lds[];  // fx_lds_bytes of the batch's widest stream
    const u32 tid = threadIdx.x;
    const u64 c = blockIdx.x / P.tiles;
    const u32 tile = blockIdx.x % P.tiles;
    if (c >= n_chunks) return;
    const u32 n = lens ? lens[c] : chunk_len;
    const u64 wk = P.wk ? P.wk[c] : P.same;
    const u32 w = (u32)(wk >> 40);
    const u32 kmax = (u32)((wk & ((1ull << 40) - 1)) - 1);  // the largest index: K - 1 <= 2^32 - 1
    const u64 total_bits = (u64)n * w;
    const u64 words = (total_bits + 31) >> 5;
    const bool fits = words * 4 <= out_stride;
    if (tile == 0 && tid == 0) {
        out_bit_off[c] = c * out_stride * 8;
        out_nbits[c] = total_bits < 0xFFFFFFFFull ? (u32)total_bits : 0xFFFFFFFFu;
        if (!fits) atomicOr(&status[c], SCL_ST_CAPACITY);
    }
    const u64 first = (u64)tile * FX_TILE;
    if (first >= n || !fits) return;
    const u32 cnt = (u32)((u64)n - first < FX_TILE ? (u64)n - first : FX_TILE);

    // symbol pieces -> LDS
    const SYM *row = sym + c * sym_stride + first;
    for (u32 p = tid; p < R::PIECES; p += FX_THREADS) {
        const u32 s0 = p * R::E;
        if (s0 >= cnt) break;
        uint4 v;
        if (s0 + R::E <= cnt) {
            v = reinterpret_cast<const uint4 *>(row)[p];
        } else {  // the row's last piece: nothing at or past symbol n
            u32 q[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 e = 0; e < R::E; ++e)
                if (s0 + e < cnt) fx_set<SYM>(q, e, (u32)row[s0 + e]);
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
        lds[p] = v;
    }
    __syncthreads();

    // a lane's 32 symbols out of LDS, all of them before any word goes back in
    const u32 *lw = reinterpret_cast<const u32 *>(lds);
    const u32 g0 = tid * FX_GROUP;
    u32 q[R::WORDS];
    if (g0 < cnt) {
#pragma unroll
        for (u32 j = 0; j < R::WORDS; ++j) q[j] = lw[tid * R::WORDS + j];
    } else {
#pragma unroll
        for (u32 j = 0; j < R::WORDS; ++j) q[j] = 0;
    }
    __syncthreads();

    u32 *wout = reinterpret_cast<u32 *>(lds) + tid * w;
    const bool bad = cnt == FX_TILE ? fx_pack_group<SYM, false>(q, g0, cnt, w, kmax, wout)
                                    : fx_pack_group<SYM, true>(q, g0, cnt, w, kmax, wout);
    if (bad) atomicOr(&status[c], SCL_ST_SYMBOL);
    __syncthreads();

    // LDS -> slot pieces; the tile starts 1024 * w bytes a tile into the slot
    const u64 tile_word0 = (u64)tile * FX_THREADS * w;
    const u64 left = words - tile_word0;
    const u32 vw = (u32)(left < (u64)FX_THREADS * w ? left : (u64)FX_THREADS * w);  // words of the stream in this tile
    u8 *base = out + c * out_stride + tile_word0 * 4;
    for (u32 p = tid; p < (FX_THREADS / 4) * w; p += FX_THREADS) {
        const u32 w0 = p * 4;
        if (w0 >= vw) break;
        if (w0 + 4 <= vw) {
            reinterpret_cast<uint4 *>(base)[p] = lds[p];
        } else {  // the stream's last piece: nothing past its last word
            for (u32 j = 0; w0 + j < vw; ++j) reinterpret_cast<u32 *>(base)[w0 + j] = lw[w0 + j];
        }
    }
}

template <class SYM>
__global__ void __launch_bounds__(FX_THREADS, 4)
    fixed_decode_kernel(FxParams P, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                        const u32 *__restrict__ in_nbits, u64 n_chunks, SYM *__restrict__ out_sym, u64 out_stride, u32 out_cap,
                        u32 *__restrict__ out_lens, u32 *__restrict__ consumed, u32 *__restrict__ status,
                        const u32 *__restrict__ lens) {
    using R = FxRow<SYM>;
    extern __shared__ __attribute__((aligned(16))) uint4 lds[];  // fx_lds_bytes of the batch's widest stream
    const u32 tid = threadIdx.x;
    const u64 c = blockIdx.x / P.tiles;
    const u32 tile = blockIdx.x % P.tiles;
    if (c >= n_chunks) return;
    const u32 n = lens ? lens[c] : out_cap;
    const u64 wk = P.wk ? P.wk[c] : P.same;
    const u32 w = (u32)(wk >> 40);
    const u32 kmax = (u32)((wk & ((1ull << 40) - 1)) - 1);  // the largest index: K - 1 <= 2^32 - 1
    const u64 off = bit_off[c];
    const u64 lim = in_size_bytes * 8;
    u64 avail = in_nbits[c];  // the stream's bits that are there to be read
    if (off >= lim) avail = 0;
    else if (avail > lim - off) avail = lim - off;
    u32 st = 0;
    u64 count = n;
    if ((u64)n * w > avail) {
        st |= SCL_ST_TRUNCATED;
        if (count > avail / w) count = avail / w;
    }
    if (n > out_cap) {
        st |= SCL_ST_CAPACITY;
        if (count > out_cap) count = out_cap;
    }
    if (tile == 0 && tid == 0) {
        out_lens[c] = (u32)count;
        consumed[c] = (u32)(count * w);
        if (st) atomicOr(&status[c], st);
    }
    const u64 first = (u64)tile * FX_TILE;
    if (first >= count) return;
    const u32 cnt = (u32)(count - first < FX_TILE ? count - first : FX_TILE);

    // the pieces that hold the tile's bit window -> LDS
    const u64 B = off + first * w;
    const u32 sh = (u32)(B & 127);
    const u64 P0 = B >> 7;
    const u32 np = (u32)((sh + (u64)cnt * w + 127) >> 7);  // <= 64 * 32 + 1; every one starts below in_size_bytes
    for (u32 p = tid; p < np; p += FX_THREADS) {
        const u64 byte0 = (P0 + p) * 16;
        uint4 v;
        if (byte0 + 16 <= in_size_bytes) {
            v = reinterpret_cast<const uint4 *>(in)[P0 + p];
        } else {  // the buffer's last, partial piece: nothing at or past in_size_bytes
            u32 q[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 e = 0; e < 16; ++e)
                if (byte0 + e < in_size_bytes) q[e >> 2] |= (u32)in[byte0 + e] << (8 * (e & 3));
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
        lds[p] = v;
    }
    __syncthreads();

    // a lane's 32 symbols: a sequential reader over the LDS words from its first bit on
    const u32 *lw = reinterpret_cast<const u32 *>(lds);
    const u32 g0 = tid * FX_GROUP;
    u32 q[R::WORDS];
#pragma unroll
    for (u32 j = 0; j < R::WORDS; ++j) q[j] = 0;
    bool bad = false;
    if (cnt == FX_TILE) bad = fx_unpack_group<SYM, false>(lw, sh + g0 * w, g0, cnt, w, kmax, q);
    else if (g0 < cnt) bad = fx_unpack_group<SYM, true>(lw, sh + g0 * w, g0, cnt, w, kmax, q);
    if (bad) atomicOr(&status[c], SCL_ST_SYMBOL);
    __syncthreads();
    {
        u32 *lo = reinterpret_cast<u32 *>(lds);
#pragma unroll
        for (u32 j = 0; j < R::WORDS; ++j) lo[tid * R::WORDS + j] = q[j];
    }
    __syncthreads();

    // LDS -> row pieces
    SYM *row = out_sym + c * out_stride + first;
    const SYM *ls = reinterpret_cast<const SYM *>(lds);
    for (u32 p = tid; p < R::PIECES; p += FX_THREADS) {
        const u32 s0 = p * R::E;
        if (s0 >= cnt) break;
        if (s0 + R::E <= cnt) {
            reinterpret_cast<uint4 *>(row)[p] = lds[p];
        } else {  // the row's last piece: nothing at or past symbol `count`
            for (u32 e = 0; s0 + e < cnt; ++e) row[s0 + e] = ls[s0 + e];
        }
    }
}

// ---- host API ------------------------------------------------------------------------------------------------------------
// widths and alphabet sizes, checked on the host and packed one word a stream
template <class SYM>
static int fx_pack(const char *what, const u32 *h_widths, const u64 *h_K, u64 n_chunks, std::vector<u64> &wk, u32 &w_max) {
    SCL_REQUIRE(h_widths && h_K, "%s: null pointer argument", what);
    wk.resize((size_t)n_chunks);
    for (u64 c = 0; c < n_chunks; ++c) {
        const u32 w = h_widths[c];
        const u64 K = h_K[c];
        SCL_REQUIRE(w >= 1 && w <= 32, "%s: stream %llu: width %u outside 1..32", what, (unsigned long long)c, w);
        SCL_REQUIRE(w <= 8 * sizeof(SYM), "%s: stream %llu: width %u needs wider symbol rows: use scl_%s_u%d", what,
                    (unsigned long long)c, w, what, w <= 16 ? 16 : 32);
        SCL_REQUIRE(K >= 1 && K <= (1ull << w), "%s: stream %llu: alphabet size %llu outside 1..2^%u", what,
                    (unsigned long long)c, (unsigned long long)K, w);
        wk[(size_t)c] = K | ((u64)w << 40);
        if (w > w_max) w_max = w;
    }
    return SCL_OK;
}

struct FxUpload {  // the packed words on the device, stream-ordered
    u64 *d = nullptr;
    hipStream_t st = nullptr;
    int put(const char *what, const std::vector<u64> &wk, hipStream_t stream) {
        st = stream;
        hipError_t e = hipMallocAsync((void **)&d, wk.size() * sizeof(u64), st);
        // (pageable host memory: the copy has left wk when the call returns)
        if (e == hipSuccess) e = hipMemcpyAsync(d, wk.data(), wk.size() * sizeof(u64), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) return SCL_OK;
        (void)hipGetLastError();
        scl_set_error("%s: uploading widths and alphabet sizes failed: %s", what, hipGetErrorString(e));
        return SCL_E_HIP;
    }
    ~FxUpload() {
        if (d) (void)hipFreeAsync(d, st);
    }
};

static int fx_params(const char *what, const std::vector<u64> &wk, hipStream_t st, FxUpload &up, FxParams &P) {
    P.wk = nullptr;
    P.same = wk[0];
    for (u64 v : wk)
        if (v != wk[0]) {
            if (int rc = up.put(what, wk, st)) return rc;
            P.wk = up.d;
            break;
        }
    return SCL_OK;
}

static int fx_grid(const char *what, u64 longest, u64 n_chunks, FxParams &P, SclGrid &grid) {
    const u64 tiles = longest ? (longest + FX_TILE - 1) / FX_TILE : 1;
    SCL_REQUIRE(tiles * n_chunks < (1ull << 31), "%s: %llu streams of up to %llu tiles: more than 2^31 - 1 workgroups", what,
                (unsigned long long)n_chunks, (unsigned long long)tiles);
    P.tiles = (u32)tiles;
    grid = {(u32)(tiles * n_chunks), FX_THREADS};
    return SCL_OK;
}

template <class SYM>
static int fx_encode_batch(const char *what, const SclEncodeArgs<SYM> &a, const u32 *h_widths, const u64 *h_K, void *stream) {
    SCL_REQUIRE(a.d_sym && a.d_out && a.d_bit_off && a.d_nbits && a.d_status && h_widths && h_K, "%s: null pointer argument",
                what);
    SCL_REQUIRE(a.out_stride % 16 == 0 && a.out_stride > 0 && a.out_stride * 8 < (1ull << 32), "%s: bad out_stride %llu", what,
                (unsigned long long)a.out_stride);
    SCL_REQUIRE(a.sym_stride * sizeof(SYM) % 16 == 0 && a.sym_stride >= a.chunk_len,
                "%s: sym_stride %llu: rows hold chunk_len symbols and start on 16-byte boundaries", what,
                (unsigned long long)a.sym_stride);
    SCL_REQUIRE((((uintptr_t)a.d_out | (uintptr_t)a.d_sym) & 15) == 0, "%s: d_out and d_sym must be 16-byte aligned", what);
    std::vector<u64> wk;
    u32 w_max = 1;
    if (int rc = fx_pack<SYM>(what, h_widths, h_K, a.n_chunks, wk, w_max)) return rc;
    FxParams P;
    SclGrid grid;
    if (int rc = fx_grid(what, a.chunk_len, a.n_chunks, P, grid)) return rc;
    grid.lds = fx_lds_bytes<SYM>(w_max);
    if (a.n_chunks == 0) return SCL_OK;
    const hipStream_t st = (hipStream_t)stream;
    FxUpload up;  // (nothing to upload when every stream has the same width and alphabet)
    if (int rc = fx_params(what, wk, st, up, P)) return rc;
    SCL_HIP_TRY(hipMemsetAsync(a.d_status, 0, a.n_chunks * sizeof(u32), st));
    scl_launch_encode(fixed_encode_kernel<SYM>, grid, st, P, a);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class SYM>
static int fx_decode_batch(const char *what, const SclDecodeArgs<SYM> &a, const u32 *d_lens, const u32 *h_widths,
                           const u64 *h_K, void *stream) {
    SCL_REQUIRE(a.d_in && a.d_bit_off && a.d_in_nbits && a.d_out_sym && a.d_out_lens && a.d_consumed && a.d_status &&
                    h_widths && h_K,
                "%s: null pointer argument", what);
    SCL_REQUIRE(a.out_stride * sizeof(SYM) % 16 == 0 && a.out_stride >= a.out_cap,
                "%s: out_stride %llu: rows hold out_cap symbols and start on 16-byte boundaries", what,
                (unsigned long long)a.out_stride);
    SCL_REQUIRE((((uintptr_t)a.d_in | (uintptr_t)a.d_out_sym) & 15) == 0, "%s: d_in and d_out_sym must be 16-byte aligned",
                what);
    std::vector<u64> wk;
    u32 w_max = 1;
    if (int rc = fx_pack<SYM>(what, h_widths, h_K, a.n_chunks, wk, w_max)) return rc;
    FxParams P;
    SclGrid grid;
    if (int rc = fx_grid(what, a.out_cap, a.n_chunks, P, grid)) return rc;
    grid.lds = fx_lds_bytes<SYM>(w_max);
    if (a.n_chunks == 0) return SCL_OK;
    const hipStream_t st = (hipStream_t)stream;
    FxUpload up;  // (nothing to upload when every stream has the same width and alphabet)
    if (int rc = fx_params(what, wk, st, up, P)) return rc;
    SCL_HIP_TRY(hipMemsetAsync(a.d_status, 0, a.n_chunks * sizeof(u32), st));
    scl_launch_decode(fixed_decode_kernel<SYM>, grid, st, P, a, d_lens);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" uint64_t scl_fixed_slot_bytes(uint64_t n_symbols, uint32_t width) {
    if (width < 1 || width > 32 || n_symbols >= (1ull << 32)) return 0;
    const u64 bits = n_symbols * width;
    if (bits >= (1ull << 32)) return 0;
    const u64 bytes = scl_round_up((bits + 31) / 32 * 4, 16);
    return bytes ? bytes : 16;
}

#define FX_ENTRY(SUFFIX, SYM)                                                                                                 \
    extern "C" int scl_fixed_encode_batch##SUFFIX(const SYM *d_sym, uint64_t sym_stride, const uint32_t *d_lens,             \
                                                  uint32_t chunk_len, const uint32_t *h_widths, const uint64_t *h_K,         \
                                                  uint64_t n_chunks, uint8_t *d_out, uint64_t out_stride,                    \
                                                  uint64_t *d_out_bit_offset, uint32_t *d_out_nbits, uint32_t *d_status,     \
                                                  void *stream) {                                                            \
        const SclEncodeArgs<SYM> a = {d_sym, sym_stride, d_lens, chunk_len, n_chunks,                                        \
                                      d_out, out_stride, d_out_bit_offset, d_out_nbits, d_status};                           \
        return fx_encode_batch<SYM>("fixed_encode_batch" #SUFFIX, a, h_widths, h_K, stream);                                 \
    }                                                                                                                         \
    extern "C" int scl_fixed_decode_batch##SUFFIX(                                                                           \
        const uint8_t *d_in, uint64_t in_size_bytes, const uint64_t *d_bit_offset, const uint32_t *d_in_nbits,               \
        const uint32_t *d_lens, const uint32_t *h_widths, const uint64_t *h_K, uint64_t n_chunks, SYM *d_out_sym,            \
        uint64_t out_stride, uint32_t out_cap, uint32_t *d_out_lens, uint32_t *d_consumed, uint32_t *d_status,               \
        void *stream) {                                                                                                       \
        const SclDecodeArgs<SYM> a = {d_in, in_size_bytes, d_bit_offset, d_in_nbits, n_chunks, d_out_sym,                    \
                                      out_stride, out_cap, d_out_lens, d_consumed, d_status};                                \
        return fx_decode_batch<SYM>("fixed_decode_batch" #SUFFIX, a, d_lens, h_widths, h_K, stream);                         \
    }
FX_ENTRY(, u8)
FX_ENTRY(_u16, u16)
FX_ENTRY(_u32, u32)
#undef FX_ENTRY

// the pair for rows of sym_bytes wide symbols, as rocprofv3 prints it (one pair per width: there is no second form)
extern "C" int scl_fixed_kernel_names(uint32_t sym_bytes, uint64_t n_chunks, char *enc, char *dec, uint64_t cap) {
    const char *what = "fixed_kernel_names";
    SCL_REQUIRE((enc || dec) && cap >= 96, "%s: null argument or a buffer below 96 bytes", what);
    SCL_REQUIRE(sym_bytes == 1 || sym_bytes == 2 || sym_bytes == 4, "%s: symbols of %u bytes: 1, 2 or 4", what, sym_bytes);
    (void)n_chunks;
    if (sym_bytes == 1)
        scl_put_names(enc, dec, (size_t)cap, "fixed_encode_kernel<unsigned char>", "fixed_decode_kernel<unsigned char>");
    else if (sym_bytes == 2)
        scl_put_names(enc, dec, (size_t)cap, "fixed_encode_kernel<unsigned short>", "fixed_decode_kernel<unsigned short>");
    else
        scl_put_names(enc, dec, (size_t)cap, "fixed_encode_kernel<unsigned int>", "fixed_decode_kernel<unsigned int>");
    return SCL_OK;
}

// ---- one stream in host memory -----------------------------------------------------------------------------------------
extern "C" int scl_fixed_encode_host(const uint32_t *h_idx, uint64_t n, uint32_t width, uint64_t K, uint8_t *h_out,
                                     uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status) {
    const char *what = "fixed_encode_host";
    SCL_REQUIRE(h_out && nbits && status && (h_idx || n == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(width >= 1 && width <= 32, "%s: width %u outside 1..32", what, width);
    SCL_REQUIRE(K >= 1 && K <= (1ull << width), "%s: alphabet size %llu outside 1..2^%u", what, (unsigned long long)K, width);
    const u64 slot = scl_fixed_slot_bytes(n, width);
    SCL_REQUIRE(slot, "%s: %llu symbols of %u bits: a stream of 2^32 bits and more", what, (unsigned long long)n, width);
    ScratchDev d_sym, d_slot, d_meta;
    int rc;
    if ((rc = d_sym.alloc(n * 4 + 16)) || (rc = d_slot.alloc(slot)) || (rc = d_meta.alloc(64))) return rc;
    if (n) SCL_HIP_TRY(hipMemcpy(d_sym.p, h_idx, n * 4, hipMemcpyHostToDevice));
    u64 *d_bit_off = (u64 *)d_meta.p;
    u32 *d_nbits = (u32 *)((u64 *)d_meta.p + 1), *d_status = d_nbits + 1;
    rc = scl_fixed_encode_batch_u32((const u32 *)d_sym.p, scl_round_up(n ? n : 1, 4), nullptr, (u32)n, &width, &K, 1,
                                    (u8 *)d_slot.p, slot, d_bit_off, d_nbits, d_status, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    u32 meta[2];
    SCL_HIP_TRY(hipMemcpy(meta, d_nbits, 8, hipMemcpyDeviceToHost));
    *nbits = meta[0];
    *status = meta[1];
    if (meta[1] & SCL_ST_CAPACITY) return SCL_OK;
    const u64 bytes = ((u64)meta[0] + 7) / 8;
    SCL_REQUIRE(bytes <= out_cap_bytes, "%s: output needs %llu bytes, capacity %llu", what, (unsigned long long)bytes,
                (unsigned long long)out_cap_bytes);
    if (bytes) SCL_HIP_TRY(hipMemcpy(h_out, d_slot.p, bytes, hipMemcpyDeviceToHost));
    return SCL_OK;
}

extern "C" int scl_fixed_decode_host(const uint8_t *h_in, uint64_t in_bit_offset, uint64_t in_nbits, uint64_t n,
                                     uint32_t width, uint64_t K, uint32_t *h_out_idx, uint64_t out_cap, uint64_t *n_out,
                                     uint64_t *consumed, uint32_t *status) {
    const char *what = "fixed_decode_host";
    SCL_REQUIRE(h_in && n_out && consumed && status && (h_out_idx || out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(width >= 1 && width <= 32, "%s: width %u outside 1..32", what, width);
    SCL_REQUIRE(K >= 1 && K <= (1ull << width), "%s: alphabet size %llu outside 1..2^%u", what, (unsigned long long)K, width);
    SCL_REQUIRE(in_nbits < (1ull << 32) && n < (1ull << 32) && out_cap < (1ull << 32), "%s: stream too large", what);
    // only the bytes that hold the stream travel
    const u64 byte0 = in_bit_offset / 8, in_bytes = (in_bit_offset % 8 + in_nbits + 7) / 8;
    ScratchDev d_in, d_out, d_meta;
    int rc;
    if ((rc = d_in.alloc(in_bytes + 16)) || (rc = d_out.alloc(out_cap * 4 + 16)) || (rc = d_meta.alloc(64))) return rc;
    if (in_bytes) SCL_HIP_TRY(hipMemcpy(d_in.p, h_in + byte0, in_bytes, hipMemcpyHostToDevice));
    const u64 h_off = in_bit_offset % 8;
    const u32 h_nb[2] = {(u32)in_nbits, (u32)n};
    u64 *d_off = (u64 *)d_meta.p;
    u32 *d_nb = (u32 *)((u64 *)d_meta.p + 1), *d_n = d_nb + 1, *d_len = d_nb + 2, *d_used = d_nb + 3, *d_status = d_nb + 4;
    SCL_HIP_TRY(hipMemset(d_meta.p, 0, 64));
    SCL_HIP_TRY(hipMemcpy(d_off, &h_off, 8, hipMemcpyHostToDevice));
    SCL_HIP_TRY(hipMemcpy(d_nb, h_nb, 8, hipMemcpyHostToDevice));
    rc = scl_fixed_decode_batch_u32((const u8 *)d_in.p, in_bytes, d_off, d_nb, d_n, &width, &K, 1, (u32 *)d_out.p,
                                    scl_round_up(out_cap ? out_cap : 1, 4), (u32)out_cap, d_len, d_used, d_status, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    u32 meta[3];
    SCL_HIP_TRY(hipMemcpy(meta, d_len, 12, hipMemcpyDeviceToHost));
    *n_out = meta[0];
    *consumed = meta[1];
    *status = meta[2];
    if (meta[0]) SCL_HIP_TRY(hipMemcpy(h_out_idx, d_out.p, (u64)meta[0] * 4, hipMemcpyDeviceToHost));
    return SCL_OK;
}
