// Wide first BWT split, sparse-prefix form: micro-benchmark (measurement only, not product code).
// Question: what does placing every rotation of a block directly at its 16-bit-prefix sub-bucket
// cost when (a) the block's non-empty 16-bit packed prefixes are mapped, order-preserving, onto dense
// bins 0..B-1 through a presence bitmap and a per-word rank table, (b) a workgroup owns one large tile
// (8 Ki / 16 Ki / 32 Ki positions) whose packed window sits in LDS, (c) the tile's elements are
// counting-sorted in LDS over the B bins as 2-byte tile-local positions and (d) stored run by run,
// the 8-byte payload (index, output byte, key bytes 2..5), the digit byte (key byte 2) or the 4-byte
// job word rebuilt from the window at store time?  Compare with the 8-bit level 0 scatter + the whole
// level 1 (histogram, scan, scatter) of bwt.hip.  wl0.hip is the round-5 form (64 Ki bins, unstaged).
//   k_w_bins + k_w_rank : the per-block prefix map          (step 1)
//   k_w_hist            : dense 16-bit count rows per tile  (step 2)
//   k_w_scatter         : the scatter                       (step 4; offsets from a host-side scan)
// All blocks have n characters of b bits; n is a multiple of the tile.
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr uint32_t NEXT_FLAG = 0x80000000u;  // offset bit 31: the sub-bucket continues as a depth-2 bucket
constexpr uint32_t BM_WORDS  = 2048;         // 65536-bit presence bitmap

struct WArgs
{
    const uint8_t*  in;      // raw blocks, n bytes each
    const uint8_t*  packed;  // packed cyclic strings, pstride bytes per block (16-byte multiple, >= n*b/8 + 48)
    const uint8_t*  inv;     // alphabet rank -> byte, 256 per block
    uint32_t*       bm;      // presence bitmaps, BM_WORDS per block
    uint16_t*       rkw;     // dense index of each bitmap word's first bit, BM_WORDS per block
    uint32_t*       nbins;   // B per block; nbins[nblocks]: the maximum
    uint16_t*       rows;    // k_w_hist: counts, bs per tile
    const uint32_t* goff;    // k_w_scatter: slot of the tile's first element of each bin (| NEXT_FLAG), bs per tile
    uint64_t*       opay;
    uint8_t*        odig;
    uint32_t*       p32;
    uint32_t        n, b, pstride, nblocks, bs, ntot;  // bs: row stride (>= every block's B); ntot = n * nblocks
};

__device__ __forceinline__ uint64_t win_bits64(const uint8_t* win, uint32_t bit)
{
    const uint32_t* w  = reinterpret_cast<const uint32_t*>(win) + (bit >> 5);
    const uint64_t  hi = ((uint64_t) __builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    const uint32_t  s  = bit & 31;
    return s ? (hi << s) | (__builtin_bswap32(w[2]) >> (32 - s)) : hi;
}

template <int TILE>
struct Geo
{
    static constexpr int THREADS = TILE / 16 < 1024 ? TILE / 16 : 1024;
    static constexpr int PT      = TILE / THREADS;
};

// tile of workgroup w, XCD-major: XCD w % 8 works through a contiguous eighth of the tile list
__device__ __forceinline__ uint32_t xcd_tile(uint32_t ntiles)
{
    const uint32_t per = (ntiles + 7) / 8;
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}

template <int TILE>
__device__ __forceinline__ void load_window(const WArgs& a, uint32_t block, uint32_t start, uint8_t* win)
{
    const uint4*   src = reinterpret_cast<const uint4*>(a.packed + (size_t) block * a.pstride + (size_t) start * a.b / 8);
    const uint32_t nq  = (TILE * a.b / 8 + 16 + 15) / 16;
    for (uint32_t i = threadIdx.x; i < nq; i += Geo<TILE>::THREADS)
        reinterpret_cast<uint4*>(win)[i] = src[i];
}

__device__ __forceinline__ uint32_t dense_of(const uint32_t* bm, const uint16_t* rkw, uint32_t p)
{
    return rkw[p >> 5] + __popc(bm[p >> 5] & ((1u << (p & 31)) - 1u));
}

template <int TILE>
__global__ void __launch_bounds__(Geo<TILE>::THREADS) k_w_bins(WArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* bm  = reinterpret_cast<uint32_t*>(smem);
    uint8_t*  win = smem + BM_WORDS * 4;
    const uint32_t tpb = a.n / TILE, t = blockIdx.x;
    if (t >= tpb * a.nblocks)
        return;
    const uint32_t block = t / tpb, start = (t % tpb) * TILE;
    load_window<TILE>(a, block, start, win);
    for (uint32_t i = threadIdx.x; i < BM_WORDS; i += Geo<TILE>::THREADS)
        bm[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < Geo<TILE>::PT; ++i)
    {
        const uint32_t e = threadIdx.x + i * Geo<TILE>::THREADS;
        const uint32_t p = (uint32_t) (win_bits64(win, e * a.b) >> 48);
        atomicOr(&bm[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < BM_WORDS; i += Geo<TILE>::THREADS)
        if (bm[i])
            atomicOr(&a.bm[(size_t) block * BM_WORDS + i], bm[i]);
}

__global__ void __launch_bounds__(1024) k_w_rank(WArgs a)
{
    __shared__ uint32_t wsum[16];
    const uint32_t  block = blockIdx.x, i = threadIdx.x, lane = i & 63, wv = i >> 6;
    const uint32_t* g     = a.bm + (size_t) block * BM_WORDS;
    const uint32_t  c0 = __popc(g[2 * i]), c1 = __popc(g[2 * i + 1]);
    uint32_t        x = c0 + c1;
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint32_t y = __shfl_up(x, d);
        if ((int) lane >= d)
            x += y;
    }
    if (lane == 63)
        wsum[wv] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < 16; ++k)
    {
        base += k < wv ? wsum[k] : 0;
        tot += wsum[k];
    }
    const uint32_t ex = base + x - c0 - c1;
    a.rkw[(size_t) block * BM_WORDS + 2 * i]     = (uint16_t) ex;
    a.rkw[(size_t) block * BM_WORDS + 2 * i + 1] = (uint16_t) (ex + c0);
    if (i == 0)
    {
        a.nbins[block] = tot;
        atomicMax(&a.nbins[a.nblocks], tot);
    }
}

// LDS of the histogram and the scatter: bitmap, rank table, bs counters, [TILE staged positions,] the window
template <int TILE>
struct Lds
{
    uint32_t* bm;
    uint16_t* rkw;
    uint32_t* cnt;
    uint16_t* st;
    uint8_t*  win;
    __device__ Lds(uint8_t* p, uint32_t bs, bool staged)
    {
        bm  = reinterpret_cast<uint32_t*>(p);
        rkw = reinterpret_cast<uint16_t*>(p + BM_WORDS * 4);
        cnt = reinterpret_cast<uint32_t*>(p + BM_WORDS * 6);
        st  = reinterpret_cast<uint16_t*>(p + BM_WORDS * 6 + bs * 4);
        win = p + BM_WORDS * 6 + bs * 4 + (staged ? TILE * 2 : 0);  // bs is a multiple of 4: 16-byte aligned
    }
};

template <int TILE>
__device__ __forceinline__ void load_map(const WArgs& a, uint32_t block, Lds<TILE>& S)
{
    for (uint32_t i = threadIdx.x; i < BM_WORDS; i += Geo<TILE>::THREADS)
    {
        S.bm[i]  = a.bm[(size_t) block * BM_WORDS + i];
        S.rkw[i] = a.rkw[(size_t) block * BM_WORDS + i];
    }
    for (uint32_t i = threadIdx.x; i < a.bs; i += Geo<TILE>::THREADS)
        S.cnt[i] = 0;
}

template <int TILE>
__global__ void __launch_bounds__(Geo<TILE>::THREADS) k_w_hist(WArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Lds<TILE>      S(smem, a.bs, false);
    const uint32_t tpb = a.n / TILE, t = blockIdx.x;
    if (t >= tpb * a.nblocks)
        return;
    const uint32_t block = t / tpb, start = (t % tpb) * TILE;
    load_window<TILE>(a, block, start, S.win);
    load_map<TILE>(a, block, S);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < Geo<TILE>::PT; ++i)
    {
        const uint32_t e = threadIdx.x + i * Geo<TILE>::THREADS;
        atomicAdd(&S.cnt[dense_of(S.bm, S.rkw, (uint32_t) (win_bits64(S.win, e * a.b) >> 48))], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.bs; i += Geo<TILE>::THREADS)
        a.rows[(size_t) t * a.bs + i] = (uint16_t) S.cnt[i];  // a count of TILE = 65536 does not occur: TILE <= 32 Ki
}

template <int TILE>
__global__ void __launch_bounds__(Geo<TILE>::THREADS) k_w_scatter(WArgs a)
{
    constexpr int THREADS = Geo<TILE>::THREADS, PT = Geo<TILE>::PT;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t wsum[THREADS / 64];
    __shared__ uint8_t  inv_s[256];
    __shared__ uint32_t prev_s;
    Lds<TILE>      S(smem, a.bs, true);
    const uint32_t tpb = a.n / TILE, ntiles = tpb * a.nblocks, t = xcd_tile(ntiles);
    if (t >= ntiles)
        return;
    const uint32_t block = t / tpb, start = (t % tpb) * TILE;
    load_window<TILE>(a, block, start, S.win);
    load_map<TILE>(a, block, S);
    if (threadIdx.x < 256)
        inv_s[threadIdx.x] = a.inv[block * 256 + threadIdx.x];
    if (threadIdx.x == 0)
        prev_s = a.in[(size_t) block * a.n + (start ? start - 1 : a.n - 1)];
    __syncthreads();
    // rank inside the tile: bin and the element's arrival number in it (order inside a run is arbitrary)
    uint32_t keep[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i)
    {
        const uint32_t e  = threadIdx.x + i * THREADS;
        const uint32_t dn = dense_of(S.bm, S.rkw, (uint32_t) (win_bits64(S.win, e * a.b) >> 48));
        keep[i]           = (dn << 16) | atomicAdd(&S.cnt[dn], 1u);
    }
    __syncthreads();
    // exclusive scan of the bin counts, in place: thread j owns bins [j * K, (j + 1) * K)
    {
        const uint32_t K = (a.bs + THREADS - 1) / THREADS, lo = threadIdx.x * K, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        uint32_t       sum = 0;
        for (uint32_t k = lo; k < min(lo + K, a.bs); ++k)
            sum += S.cnt[k];
        uint32_t x = sum;
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t y = __shfl_up(x, d);
            if ((int) lane >= d)
                x += y;
        }
        if (lane == 63)
            wsum[wv] = x;
        __syncthreads();
        uint32_t run = x - sum;
        for (uint32_t k = 0; k < wv; ++k)
            run += wsum[k];
        for (uint32_t k = lo; k < min(lo + K, a.bs); ++k)
        {
            const uint32_t c = S.cnt[k];
            S.cnt[k]         = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PT; ++i)
        S.st[S.cnt[keep[i] >> 16] + (keep[i] & 0xFFFFu)] = (uint16_t) (threadIdx.x + i * THREADS);
    __syncthreads();
    // bin -> (slot of the tile's run) - (staged position of the run), modulo 2^31, the flag kept in bit 31
    for (uint32_t i = threadIdx.x; i < a.bs; i += THREADS)
    {
        const uint32_t g = a.goff[(size_t) t * a.bs + i];
        S.cnt[i]         = (((g & ~NEXT_FLAG) - S.cnt[i]) & ~NEXT_FLAG) | (g & NEXT_FLAG);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PT; ++i)
    {
        const uint32_t q    = threadIdx.x + i * THREADS;
        const uint32_t e    = S.st[q];
        const uint64_t kk   = win_bits64(S.win, e * a.b);  // key bytes 0..7
        const uint32_t g    = S.cnt[dense_of(S.bm, S.rkw, (uint32_t) (kk >> 48))];
        const uint32_t slot = (g + q) & ~NEXT_FLAG;
        const uint32_t lb   = e ? inv_s[(uint32_t) (win_bits64(S.win, (e - 1) * a.b) >> (64 - a.b))] : prev_s;
        const uint32_t pos  = start + e;
        if (slot < a.ntot)
        {
            if (g & NEXT_FLAG)
            {
                a.opay[slot] = ((kk << 16) & 0xFFFFFFFF00000000ull) | ((uint64_t) lb << 24) | pos;  // key bytes 2..5
                a.odig[slot] = (uint8_t) (kk >> 40);                                                 // key byte 2: the depth-2 digit
            }
            else
                a.p32[slot] = (lb << 24) | pos;
        }
    }
}

template <int TILE>
static int launch(int which, const WArgs& a, hipStream_t s)
{
    const uint32_t ntiles = a.n / TILE * a.nblocks;
    const uint32_t win    = TILE * a.b / 8 + 32;
    if (a.n % TILE || a.bs % 4)
        return -2;
    if (which == 0)
    {
        hipLaunchKernelGGL(k_w_bins<TILE>, dim3(ntiles), dim3(Geo<TILE>::THREADS), BM_WORDS * 4 + win, s, a);
        hipLaunchKernelGGL(k_w_rank, dim3(a.nblocks), dim3(1024), 0, s, a);
    }
    else if (which == 1)
    {
        const uint32_t lds = BM_WORDS * 6 + a.bs * 4 + win;
        if (hipFuncSetAttribute((const void*) k_w_hist<TILE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            return -4;
        hipLaunchKernelGGL(k_w_hist<TILE>, dim3(ntiles), dim3(Geo<TILE>::THREADS), lds, s, a);
    }
    else
    {
        const uint32_t lds = BM_WORDS * 6 + a.bs * 4 + TILE * 2 + win;
        if (lds > 160 * 1024 - 2048)
            return -3;
        if (hipFuncSetAttribute((const void*) k_w_scatter<TILE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            return -4;
        hipLaunchKernelGGL(k_w_scatter<TILE>, dim3((ntiles + 7) / 8 * 8), dim3(Geo<TILE>::THREADS), lds, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// which: 0 prefix map, 1 histogram, 2 scatter; tile: 8192 / 16384 / 32768
extern "C" int wl0w_launch(int which, int tile, const WArgs* a, void* stream)
{
    hipStream_t s = (hipStream_t) stream;
    switch (tile)
    {
    case 8192: return launch<8192>(which, *a, s);
    case 16384: return launch<16384>(which, *a, s);
    case 32768: return launch<32768>(which, *a, s);
    }
    return -2;
}

extern "C" unsigned wl0w_scatter_lds(int tile, unsigned b, unsigned bs) { return BM_WORDS * 6 + bs * 4 + tile * 2 + tile * b / 8 + 32; }
