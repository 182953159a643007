// scl_typical.hip -- the typical-set code of the reference (typical_set_coder.py) for gfx950: the tables built on the device,
// and ONE block of chunks coded by the whole grid.  The fourth user of scl_bit_block.h.
//
// tables   The reference enumerates X^n in Python, twice; here the N = K^n tuples are classified independently, a prefix count
//          over the flags numbers the typical ones.  The shape of the block encoder (tile counts, one-workgroup scan, tile emit):
//          ts_tile_count   a workgroup classifies its tile of TS_TILE tuples (scl_typical_rule.h, 16 a thread) and stores the
//                          number of typical ones
//          ts_scan         ONE workgroup: scl_block_scan_array over the tile counts; the total is `count`
//          ts_tile_rank    classifies again, scans inside the tile: rank[t] = the number of a typical tuple (SCL_TYPICAL_NONE
//                          otherwise), inv[rank[t]] = t
//          rank[N] and inv[count] are plain uint32 arrays in HBM, read through the cache by the coders.
// encode   the value policy TsEnc: a "value" is a chunk of n symbols; the thread reads its 16 chunks (contiguous symbols),
//          forms t by Horner's rule and gathers rank[t]: {rank, 1 + bt} or {1 << bo | t, 1 + bo}.  A symbol >= K is
//          SCL_ST_SYMBOL, coded as symbol 0, as in scl_prefix_block.hip.
// decode   the codeword policy TsCode: the flag is the top bit of the look, the index the bt or bo bits behind it; the walk
//          needs the length alone, the write kernel gathers inv[index].  pfb_write_body stores one uint32 tuple per codeword
//          into scratch; ts_unpack writes its n base-K digits, ts_result turns the result's chunk count into symbols.
// As in scl_prefix_block.hip no kernel waits on another workgroup: every dependency between workgroups is a kernel boundary.
// fp64 appears in the table kernels alone: n additions and one division a tuple, 2^24 tuples at the most.  DESIGN.md 3.5.5.
#include <cmath>

#include "scl_bit_block.h"
#include "scl_typical_rule.h"

#define TS_THREADS 256
#define TS_PER_THREAD 16u
#define TS_TILE (TS_THREADS * TS_PER_THREAD)  // 4096 tuples a workgroup
#define TS_SCAN_THREADS 1024
#define TS_MAX_N (1u << 24)  // symbols a chunk: above it only K = 1 would pass the tuple cap

struct TsDev {  // what the kernels take by value
    const double *nlp;  // [K]
    u32 *rank;          // [N]
    u32 *inv;           // [max(count, 1)]
    double entropy, eps;
    u32 K, n, N, top;   // top = K^(n-1)
    u32 count, bt, bo;  // bt: SCL_TYPICAL_NONE for an empty typical set
};

struct scl_typical_model {
    int device = 0;
    TsDev dev = {};
    double *d_nlp = nullptr;
    u32 *d_rank = nullptr, *d_inv = nullptr;
};

// ---- the tables -----------------------------------------------------------------------------------------------------------
// the flags of the thread's TS_PER_THREAD consecutive tuples (bit j: tuple first + j is typical) -> their count
__device__ __forceinline__ u32 ts_classify(const TsDev &T, u32 first, u32 &flags) {
    flags = 0;
#pragma unroll 1
    for (u32 j = 0; j < TS_PER_THREAD; ++j) {
        const u32 t = first + j;
        if (t < T.N && scl_typical_rule(T.nlp, T.K, T.n, T.top, T.entropy, T.eps, t)) flags |= 1u << j;
    }
    return (u32)__popc(flags);
}

__global__ void __launch_bounds__(TS_THREADS) ts_tile_count_kernel(TsDev T, u32 *__restrict__ tile_count) {
    __shared__ u32 s_wave[TS_THREADS / 64];
    u32 flags, total;
    const u32 mine = ts_classify(T, blockIdx.x * TS_TILE + threadIdx.x * TS_PER_THREAD, flags);
    (void)scl_block_scan_excl<u32, TS_THREADS, SclScanSum>(mine, s_wave, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TS_SCAN_THREADS) ts_scan_kernel(u32 *__restrict__ tile_count, u32 n_tiles, u32 *__restrict__ count) {
    __shared__ u32 s_wave[TS_SCAN_THREADS / 64];
    const u32 total = scl_block_scan_array<u32, TS_SCAN_THREADS, SclScanSum>(tile_count, n_tiles, s_wave);
    if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(TS_THREADS) ts_tile_rank_kernel(TsDev T, const u32 *__restrict__ tile_off) {
    __shared__ u32 s_wave[TS_THREADS / 64];
    const u32 first = blockIdx.x * TS_TILE + threadIdx.x * TS_PER_THREAD;
    u32 flags, total;
    const u32 mine = ts_classify(T, first, flags);
    u32 r = tile_off[blockIdx.x] + scl_block_scan_excl<u32, TS_THREADS, SclScanSum>(mine, s_wave, &total);
#pragma unroll 1
    for (u32 j = 0; j < TS_PER_THREAD; ++j) {
        const u32 t = first + j;
        if (t >= T.N) break;
        const bool typical = (flags >> j) & 1u;
        T.rank[t] = typical ? r : SCL_TYPICAL_NONE;
        if (typical) {
            if (r < T.count) T.inv[r] = t;  // (always: the count is the sum of the same flags)
            ++r;
        }
    }
}

static u32 ts_tiles(u32 N) { return (N + TS_TILE - 1) / TS_TILE; }

static int ts_check_params(const char *what, const double *h_nlp, u32 K, u32 n, double entropy, double eps, u32 *N) {
    SCL_REQUIRE(h_nlp, "%s: null pointer argument", what);
    SCL_REQUIRE(K >= 1 && K <= SCL_MAX_ALPHABET, "%s: alphabet of %u symbols outside 1..65536", what, K);
    SCL_REQUIRE(n >= 1 && n <= TS_MAX_N, "%s: chunks of %u symbols outside 1..2^24", what, n);
    u64 tuples = 1;
    for (u32 i = 0; i < n && K > 1; ++i) {
        tuples *= K;
        SCL_REQUIRE(tuples <= SCL_TYPICAL_MAX_TUPLES, "%s: %u^%u tuples: more than 2^24 are not enumerated", what, K, n);
    }
    for (u32 s = 0; s < K; ++s) SCL_REQUIRE(std::isfinite(h_nlp[s]), "%s: nlp[%u] is not finite", what, s);
    SCL_REQUIRE(std::isfinite(entropy) && std::isfinite(eps), "%s: entropy and eps must be finite", what);
    *N = (u32)tuples;
    return SCL_OK;
}

extern "C" uint32_t scl_typical_index_bits_host(uint64_t x) { return scl_typical_index_bits(x); }

extern "C" int scl_typical_table_host(const double *h_nlp, uint32_t K, uint32_t n, double entropy, double eps, uint32_t *h_rank,
                                      uint32_t *count) {
    u32 N;
    if (int rc = ts_check_params("typical_table_host", h_nlp, K, n, entropy, eps, &N)) return rc;
    SCL_REQUIRE(count, "typical_table_host: null pointer argument");
    const u32 top = scl_typical_top(K, n);
    u32 r = 0;
    for (u32 t = 0; t < N; ++t) {
        const bool typical = scl_typical_rule(h_nlp, K, n, top, entropy, eps, t);
        if (h_rank) h_rank[t] = typical ? r : SCL_TYPICAL_NONE;
        r += typical ? 1u : 0u;
    }
    *count = r;
    return SCL_OK;
}

extern "C" void scl_typical_model_destroy(scl_typical_model *m) {
    if (!m) return;
    if (m->d_nlp) (void)hipFree(m->d_nlp);
    if (m->d_rank) (void)hipFree(m->d_rank);
    if (m->d_inv) (void)hipFree(m->d_inv);
    delete m;
}

static int ts_build_tables(scl_typical_model *m, const double *h_nlp) {
    const char *what = "typical_model_create: device table";
    TsDev &T = m->dev;
    const u32 n_tiles = ts_tiles(T.N);
    ScratchDev d_tiles;  // tile counts, then the count
    if (int rc = d_tiles.alloc((u64)(n_tiles + 1) * 4)) return rc;
    u32 *tile_count = (u32 *)d_tiles.p, *d_count = tile_count + n_tiles;
    if (int rc = scl_upload(&m->d_nlp, h_nlp, T.K, what)) return rc;
    if (int rc = scl_upload(&m->d_rank, (const u32 *)nullptr, 0, what, T.N)) return rc;
    T.nlp = m->d_nlp;
    T.rank = m->d_rank;
    // every buffer the kernels fill holds 0xA5 in front of them: an entry they miss is not a plausible number
    SCL_HIP_TRY(hipMemset(d_tiles.p, 0xA5, (u64)(n_tiles + 1) * 4));
    SCL_HIP_TRY(hipMemset(m->d_rank, 0xA5, (u64)T.N * 4));
    hipLaunchKernelGGL(ts_tile_count_kernel, dim3(n_tiles), dim3(TS_THREADS), 0, nullptr, T, tile_count);
    hipLaunchKernelGGL(ts_scan_kernel, dim3(1), dim3(TS_SCAN_THREADS), 0, nullptr, tile_count, n_tiles, d_count);
    SCL_HIP_TRY(hipGetLastError());
    SCL_HIP_TRY(hipMemcpy(&T.count, d_count, 4, hipMemcpyDeviceToHost));  // (waits for the two kernels)
    SCL_REQUIRE(T.count <= T.N, "typical_model_create: the device counted %u typical tuples of %u", T.count, T.N);
    if (int rc = scl_upload(&m->d_inv, (const u32 *)nullptr, 0, what, T.count)) return rc;
    T.inv = m->d_inv;
    SCL_HIP_TRY(hipMemset(m->d_inv, 0xA5, (u64)(T.count ? T.count : 1) * 4));
    T.bt = scl_typical_index_bits(T.count);
    T.bo = scl_typical_index_bits(T.N);
    hipLaunchKernelGGL(ts_tile_rank_kernel, dim3(n_tiles), dim3(TS_THREADS), 0, nullptr, T, (const u32 *)tile_count);
    SCL_HIP_TRY(hipGetLastError());
    SCL_HIP_TRY(hipDeviceSynchronize());  // d_tiles is freed on return
    return SCL_OK;
}

extern "C" int scl_typical_model_create(const double *h_nlp, uint32_t K, uint32_t n, double entropy, double eps,
                                        scl_typical_model **out) {
    SCL_REQUIRE(out, "typical_model_create: null output");
    *out = nullptr;
    u32 N;
    if (int rc = ts_check_params("typical_model_create", h_nlp, K, n, entropy, eps, &N)) return rc;
    scl_typical_model *m = new scl_typical_model();
    m->device = scl_current_device();
    m->dev.K = K;
    m->dev.n = n;
    m->dev.N = N;
    m->dev.top = scl_typical_top(K, n);
    m->dev.entropy = entropy;
    m->dev.eps = eps;
    if (int rc = ts_build_tables(m, h_nlp)) {
        scl_typical_model_destroy(m);
        return rc;
    }
    *out = m;
    return SCL_OK;
}

extern "C" int scl_typical_model_info(const scl_typical_model *m, scl_typical_info *info) {
    SCL_REQUIRE(m && info, "typical_model_info: null argument");
    info->N = m->dev.N;
    info->count = m->dev.count;
    info->bt = m->dev.bt;
    info->bo = m->dev.bo;
    info->K = m->dev.K;
    info->n = m->dev.n;
    info->device = m->device;
    info->reserved = 0;
    return SCL_OK;
}

extern "C" int scl_typical_model_tables(const scl_typical_model *m, uint32_t *h_rank, uint32_t *h_inv) {
    SCL_REQUIRE(m, "typical_model_tables: null argument");
    if (int rc = scl_check_device(m->device, "typical_model_tables")) return rc;
    if (h_rank) SCL_HIP_TRY(hipMemcpy(h_rank, m->d_rank, (u64)m->dev.N * 4, hipMemcpyDeviceToHost));
    if (h_inv && m->dev.count) SCL_HIP_TRY(hipMemcpy(h_inv, m->d_inv, (u64)m->dev.count * 4, hipMemcpyDeviceToHost));
    return SCL_OK;
}

// ---- encode ---------------------------------------------------------------------------------------------------------------
// the value policy of pfb_tile_bits_body / pfb_encode_tile_body: a value is a chunk of n symbols
template <typename SYM>
struct TsEnc {
    const TsDev &T;
    const SYM *__restrict__ sym;
    u64 n_chunks;
    const u64 *tile_off;  // the scanned tile sums (tile-emit)
    static constexpr bool kTables = false;
    static constexpr u32 kFault = SCL_ST_SYMBOL;

    __device__ __forceinline__ void load() const {}
    __device__ __forceinline__ u64 tile_base(u32 block) const { return tile_off[block]; }
    // the {bits, length} of the thread's PFB_PER_THREAD consecutive chunks (length 0 past the end of the block)
    __device__ __forceinline__ u32 codes(u32 block, uint2 (&e)[PFB_PER_THREAD], u32 &bad) const {
        const u64 first = (u64)block * PFB_TILE + threadIdx.x * PFB_PER_THREAD;
        const u32 n = T.n, K = T.K;
        // the thread's 16 chunks are 16 n contiguous symbols, a whole number of 16-byte pieces that start on a 16-byte
        // boundary if d_sym does: they are read a piece at a time (neighbouring lanes are 16 n symbols apart, so a load of single
        // symbols touches as many cache lines and brings 16 times less).  The last tile's partial threads read symbol by symbol.
        constexpr u32 kPiece = 16 / sizeof(SYM);  // symbols a piece
        const SYM *mine = sym + first * n;        // (not dereferenced past the block)
        const bool whole = first + PFB_PER_THREAD <= n_chunks && (((uintptr_t)mine) & 15) == 0;
        uint4 piece = make_uint4(0u, 0u, 0u, 0u);
        u32 q = 0;  // symbols of the thread's range taken so far
        u32 bits = 0;
#pragma unroll
        for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
            uint2 c = make_uint2(0u, 0u);
            if (whole || first + j < n_chunks) {
                u32 t = 0;
                for (u32 i = 0; i < n; ++i, ++q) {  // Horner: t < K^n as long as every digit is below K
                    u32 x;
                    if (whole) {
                        const u32 at = (q & (kPiece - 1)) * (u32)sizeof(SYM);  // byte of the piece
                        if (at == 0) piece = *reinterpret_cast<const uint4 *>(mine + q);
                        const u32 w = (at >> 2) == 0 ? piece.x : (at >> 2) == 1 ? piece.y : (at >> 2) == 2 ? piece.z : piece.w;
                        x = (w >> (8u * (at & 3u))) & (sizeof(SYM) == 1 ? 0xFFu : 0xFFFFu);
                    } else {
                        x = mine[q];
                    }
                    if (x >= K) {
                        bad = 1;
                        x = 0;
                    }
                    t = t * K + x;
                }
                const u32 r = T.rank[t];
                c = r != SCL_TYPICAL_NONE ? make_uint2(r, 1u + T.bt) : make_uint2((1u << T.bo) | t, 1u + T.bo);
            }
            e[j] = c;
            bits += c.y;
        }
        return bits;
    }
};

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    ts_tile_bits_kernel(TsDev T, const SYM *__restrict__ sym, u64 n_chunks, u64 *__restrict__ tile_bits, u32 *__restrict__ status) {
    pfb_tile_bits_body(TsEnc<SYM>{T, sym, n_chunks, nullptr}, tile_bits, status);
}

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    ts_encode_tile_kernel(TsDev T, const SYM *__restrict__ sym, u64 n_chunks, const u64 *__restrict__ tile_off,
                          PfbEncScratch *__restrict__ head, u32 *__restrict__ out32, u64 tail_index) {
    pfb_encode_tile_body(TsEnc<SYM>{T, sym, n_chunks, tile_off}, head, out32, tail_index);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
// the codeword policy of pfb_sync_body / pfb_write_body: the flag, then an index of bt or bo bits (either may be 0 bits)
struct TsCode {
    const TsDev &T;
    __device__ __forceinline__ void load() const {}
    __device__ __forceinline__ u32 len_gcd() const {
        u32 a = 1u + T.bo, b = T.bt == SCL_TYPICAL_NONE ? 0u : 1u + T.bt;
        while (b) {
            const u32 r = a % b;
            a = b;
            b = r;
        }
        return a;
    }
    __device__ __forceinline__ u32 codeword(u32 bits, u32 rem, u32 &len, u32 &sym) const {
        const bool other = bits >> 31;
        const u32 w = other ? T.bo : T.bt;
        if (!other && w == SCL_TYPICAL_NONE) return PFB_END_STATE;  // flag 0 and no typical set
        len = 1u + w;
        if (len > rem) return PFB_END_TRUNC;
        const u32 index = w ? (bits << 1) >> (32u - w) : 0u;  // (w <= 24)
        if (index >= (other ? T.N : T.count)) return PFB_END_STATE;
        sym = other ? index : T.inv[index];
        return PFB_END_EXIT;
    }
};

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ts_sync_kernel(TsDev T, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub, u64 n_groups,
                   PfbDecScratch sc, u32 pass) {
    pfb_sync_body(TsCode{T}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, n_groups, sc.head, sc.g, pass);
}

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ts_write_kernel(TsDev T, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                    PfbDecScratch sc, u32 *__restrict__ tuples, u64 chunk_cap, PfbDecResult *__restrict__ result) {
    pfb_write_body(TsCode{T}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, sc.head, sc.g, tuples, chunk_cap,
                   &result->consumed);
}

// one thread a chunk: the n base-K digits of its tuple, position 0 first; result->n_out still counts chunks
template <typename SYM>
__global__ void __launch_bounds__(TS_THREADS)
    ts_unpack_kernel(u32 K, u32 n, const u32 *__restrict__ tuples, u64 chunk_cap, const PfbDecResult *__restrict__ result,
                     SYM *__restrict__ out) {
    const u64 c = (u64)blockIdx.x * TS_THREADS + threadIdx.x;
    const u64 n_chunks = result->n_out < chunk_cap ? result->n_out : chunk_cap;
    if (c >= n_chunks) return;
    u32 t = tuples[c];
    SYM *p = out + c * n;
    for (u32 i = n; i-- > 0;) {
        const u32 q = K > 1 ? t / K : 0u;
        p[i] = (SYM)(t - q * K);
        t = q;
    }
}

static __global__ void ts_result_kernel(u32 n, PfbDecResult *__restrict__ result) { result->n_out *= n; }

// ---- host API -------------------------------------------------------------------------------------------------------------
static u32 ts_min_len(const TsDev &T) { return T.bt == SCL_TYPICAL_NONE ? 1u + T.bo : 1u + (T.bt < T.bo ? T.bt : T.bo); }
// the chunks a stream of nbits can hold, the scratch of the decoder proper (the tuples lie behind it)
static u64 ts_max_chunks(const TsDev &T, u64 nbits) { return nbits / ts_min_len(T); }
static u64 ts_dec_head(u64 nbits) { return scl_round_up(pfb_dec_scratch(nbits), 256); }

extern "C" uint64_t scl_typical_block_scratch_bytes(const scl_typical_model *m, uint64_t n_symbols, uint64_t in_nbits) {
    if (!m) return 0;
    const u64 e = pfb_enc_scratch(n_symbols / m->dev.n), d = ts_dec_head(in_nbits) + (ts_max_chunks(m->dev, in_nbits) + 1) * 4;
    return scl_round_up(e > d ? e : d, 256);
}

PFB_RESULT_IS(scl_typical_block_result);
static const PfbWords TS_WORDS = {"chunks", "scl_typical_block_scratch_bytes",
                                  "d_out must be 4-byte, d_scratch and d_nbits 8-byte aligned, d_sym as its symbols",
                                  "d_in must be 4-byte, d_scratch and d_result 8-byte aligned, d_out_sym as its symbols"};

template <class SYM>
static int ts_check_model(const char *what, const scl_typical_model *m) {
    SCL_REQUIRE(m, "%s: null pointer argument", what);
    SCL_REQUIRE(sizeof(SYM) == 2 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K, what);
    return scl_check_device(m->device, what);
}

// the bytes of the longest stream of n_chunks chunks: the flag and bo bits each (count <= N, so bt <= bo)
static u64 ts_reach(const scl_typical_model *m, u64 n_chunks) { return scl_round_up((n_chunks * (1 + m->dev.bo) + 7) / 8, 4); }

// a.n counts CHUNKS here and below: the value of the shared launchers is a chunk
template <class SYM>
static int ts_encode(const char *what, const scl_typical_model *m, const PfbEncodeArgs &a, hipStream_t st) {
    if (int rc = ts_check_model<SYM>(what, m)) return rc;
    const SYM *d_sym = (const SYM *)a.d_val;
    return pfb_encode_launch<0u>(
        what, TS_WORDS, a, ((uintptr_t)d_sym & (sizeof(SYM) - 1)) == 0, ts_reach(m, a.n), st,
        [&](dim3 grid, u64 *tile_bits, u32 *status) {
            hipLaunchKernelGGL(ts_tile_bits_kernel<SYM>, grid, dim3(PFB_THREADS), 0, st, m->dev, d_sym, a.n, tile_bits, status);
        },
        [&](dim3 grid, const u64 *tile_off, PfbEncScratch *head, u32 *out32, u64 tail_index) {
            hipLaunchKernelGGL(ts_encode_tile_kernel<SYM>, grid, dim3(PFB_THREADS), 0, st, m->dev, d_sym, a.n, tile_off, head,
                               out32, tail_index);
        });
}

// a.out_cap counts SYMBOLS; the tuples of at most chunk_cap chunks go to the scratch behind the decoder's own
template <class SYM>
static int ts_decode(const char *what, const scl_typical_model *m, const PfbDecodeArgs &a, hipStream_t st) {
    if (int rc = ts_check_model<SYM>(what, m)) return rc;
    const TsDev &T = m->dev;
    SCL_REQUIRE(a.in_nbits < (1ull << 46), "%s: stream of %llu bits: 2^46 and more are not coded", what,
                (unsigned long long)a.in_nbits);
    const u64 fits = ts_max_chunks(T, a.in_nbits), asked = a.out_cap / T.n;
    // no stream of in_nbits holds more than `fits` chunks: a larger cap is `fits` + 1, which bounds the tuples in scratch and
    // is still never reached (bits left behind `fits` chunks are a cut or a bad codeword, not SCL_ST_CAPACITY)
    const u64 chunk_cap = asked <= fits ? asked : fits + 1;
    const u64 need = ts_dec_head(a.in_nbits) + (fits + 1) * 4;
    SCL_REQUIRE(a.d_scratch && a.scratch_bytes >= need, "%s: scratch of %llu bytes, %s asks for %llu", what,
                (unsigned long long)a.scratch_bytes, TS_WORDS.scratch_fn, (unsigned long long)need);
    u32 *tuples = (u32 *)((u8 *)a.d_scratch + ts_dec_head(a.in_nbits));
    PfbDecodeArgs b = a;
    b.d_out = tuples;  // never null, so that out_cap = 0 with a null d_out_sym passes the shared check
    b.out_cap = chunk_cap;
    SCL_REQUIRE(a.d_out || a.out_cap == 0, "%s: null pointer argument", what);
    int rc = pfb_decode_launch<SCL_ST_STATE>(
        what, TS_WORDS, b, ((uintptr_t)a.d_out & (sizeof(SYM) - 1)) == 0, st,
        [&](dim3 grid, u64 n_sub, u64 n_groups, const PfbDecScratch &sc, u32 pass) {
            hipLaunchKernelGGL(ts_sync_kernel, grid, dim3(PFB_THREADS), 0, st, T, a.d_in, a.in_size_bytes, a.in_bit_offset,
                               a.in_nbits, n_sub, n_groups, sc, pass);
        },
        [&](dim3 grid, u64 n_sub, const PfbDecScratch &sc) {
            hipLaunchKernelGGL(ts_write_kernel, grid, dim3(PFB_THREADS), 0, st, T, a.d_in, a.in_size_bytes, a.in_bit_offset,
                               a.in_nbits, n_sub, sc, tuples, chunk_cap, a.d_result);
        });
    if (rc || a.in_nbits == 0) return rc;
    if (chunk_cap) {
        const u64 blocks = (chunk_cap + TS_THREADS - 1) / TS_THREADS;
        SCL_REQUIRE(blocks < (1ull << 31), "%s: %llu chunks: more than 2^39 - 1 are not unpacked", what,
                    (unsigned long long)chunk_cap);
        hipLaunchKernelGGL(ts_unpack_kernel<SYM>, dim3((u32)blocks), dim3(TS_THREADS), 0, st, T.K, T.n, (const u32 *)tuples,
                           chunk_cap, (const PfbDecResult *)a.d_result, (SYM *)a.d_out);
    }
    hipLaunchKernelGGL(ts_result_kernel, dim3(1), dim3(1), 0, st, T.n, a.d_result);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class SYM>
static int ts_encode_symbols(const char *what, const scl_typical_model *m, const SYM *d_sym, u64 n_symbols, u8 *d_out,
                             u64 out_cap_bytes, u64 *d_nbits, u32 *d_status, void *d_scratch, u64 scratch_bytes, void *stream) {
    SCL_REQUIRE(m, "%s: null pointer argument", what);
    SCL_REQUIRE(n_symbols % m->dev.n == 0, "%s: %llu symbols are no multiple of the chunk length %u", what,
                (unsigned long long)n_symbols, m->dev.n);
    return ts_encode<SYM>(what, m, {d_sym, n_symbols / m->dev.n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch, scratch_bytes},
                          (hipStream_t)stream);
}

extern "C" int scl_typical_encode_block(const scl_typical_model *m, const uint8_t *d_sym, uint64_t n_symbols, uint8_t *d_out,
                                        uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                        uint64_t scratch_bytes, void *stream) {
    return ts_encode_symbols<u8>("typical_encode_block", m, d_sym, n_symbols, d_out, out_cap_bytes, d_nbits, d_status, d_scratch,
                                 scratch_bytes, stream);
}

extern "C" int scl_typical_encode_block_u16(const scl_typical_model *m, const uint16_t *d_sym, uint64_t n_symbols, uint8_t *d_out,
                                            uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                            uint64_t scratch_bytes, void *stream) {
    return ts_encode_symbols<u16>("typical_encode_block_u16", m, d_sym, n_symbols, d_out, out_cap_bytes, d_nbits, d_status,
                                  d_scratch, scratch_bytes, stream);
}

extern "C" int scl_typical_decode_block(const scl_typical_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                        uint64_t in_bit_offset, uint64_t in_nbits, uint8_t *d_out_sym, uint64_t out_cap,
                                        scl_typical_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                        void *stream) {
    return ts_decode<u8>("typical_decode_block", m,
                         {d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, (PfbDecResult *)d_result, d_scratch,
                          scratch_bytes},
                         (hipStream_t)stream);
}

extern "C" int scl_typical_decode_block_u16(const scl_typical_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                            uint64_t in_bit_offset, uint64_t in_nbits, uint16_t *d_out_sym, uint64_t out_cap,
                                            scl_typical_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                            void *stream) {
    return ts_decode<u16>("typical_decode_block_u16", m,
                          {d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, (PfbDecResult *)d_result, d_scratch,
                           scratch_bytes},
                          (hipStream_t)stream);
}

// ---- one block in host memory (the staging: scl_bit_block.h); the status goes back to the caller --------------------------
template <class SYM>
static int ts_encode_host(const char *what, const scl_typical_model *m, const SYM *h_sym, u64 n_symbols, u8 *h_out,
                          u64 out_cap_bytes, u64 *nbits, u32 *status) {
    if (int rc = ts_check_model<SYM>(what, m)) return rc;
    SCL_REQUIRE(h_out && nbits && status && (h_sym || n_symbols == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(n_symbols % m->dev.n == 0, "%s: %llu symbols are no multiple of the chunk length %u", what,
                (unsigned long long)n_symbols, m->dev.n);
    const u64 n_chunks = n_symbols / m->dev.n;
    return pfb_encode_staged(what, TS_WORDS, h_sym, n_chunks, (u64)m->dev.n * sizeof(SYM), ts_reach(m, n_chunks), h_out,
                             out_cap_bytes, nbits, status, [&](const PfbEncodeArgs &a) { return ts_encode<SYM>(what, m, a, nullptr); });
}

template <class SYM>
static int ts_decode_host(const char *what, const scl_typical_model *m, const u8 *h_in, u64 in_nbits, SYM *h_out_sym, u64 out_cap,
                          u64 *n_out, u64 *consumed, u32 *status) {
    if (int rc = ts_check_model<SYM>(what, m)) return rc;
    SCL_REQUIRE(h_in && n_out && consumed && status && (h_out_sym || out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(in_nbits < (1ull << 46), "%s: stream of %llu bits: 2^46 and more are not coded", what, (unsigned long long)in_nbits);
    // the staging sizes the decoder's own scratch; the tuples need more: this call brings the whole of it
    const u64 scratch_bytes = scl_typical_block_scratch_bytes(m, 0, in_nbits);
    ScratchDev d_scr;
    if (int rc = d_scr.alloc(scratch_bytes)) return rc;
    return pfb_decode_staged(what, h_in, in_nbits, h_out_sym, sizeof(SYM), out_cap, true, n_out, consumed, status,
                             [&](const PfbDecodeArgs &a) {
                                 PfbDecodeArgs b = a;
                                 b.d_scratch = d_scr.p;
                                 b.scratch_bytes = scratch_bytes;
                                 return ts_decode<SYM>(what, m, b, nullptr);
                             });
}

extern "C" int scl_typical_encode_block_host(const scl_typical_model *m, const uint8_t *h_sym, uint64_t n_symbols, uint8_t *h_out,
                                             uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status) {
    return ts_encode_host<u8>("typical_encode_block_host", m, h_sym, n_symbols, h_out, out_cap_bytes, nbits, status);
}

extern "C" int scl_typical_encode_block_host_u16(const scl_typical_model *m, const uint16_t *h_sym, uint64_t n_symbols,
                                                 uint8_t *h_out, uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status) {
    return ts_encode_host<u16>("typical_encode_block_host_u16", m, h_sym, n_symbols, h_out, out_cap_bytes, nbits, status);
}

extern "C" int scl_typical_decode_block_host(const scl_typical_model *m, const uint8_t *h_in, uint64_t in_nbits, uint8_t *h_out_sym,
                                             uint64_t out_cap, uint64_t *n_out, uint64_t *consumed, uint32_t *status) {
    return ts_decode_host<u8>("typical_decode_block_host", m, h_in, in_nbits, h_out_sym, out_cap, n_out, consumed, status);
}

extern "C" int scl_typical_decode_block_host_u16(const scl_typical_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                                 uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                                                 uint32_t *status) {
    return ts_decode_host<u16>("typical_decode_block_host_u16", m, h_in, in_nbits, h_out_sym, out_cap, n_out, consumed, status);
}
