// mvsv_bm_census.hip — StereoBM on a census matching cost.
//
// mvsv_bm's pipeline with the pixel cost swapped: where StereoBM takes
// |Lf(y, xl) - Rf(y, xr)| on prefiltered bytes, this takes
// popcount(T_L(y, xl) ^ T_R(y, xr)) on the census descriptors of mvsv_census.hip.
// The column pairs (xl, xr) are the virtual-column clamps of mvsv_bm.hip; the
// window sum, argmin, uniqueness test, parabola fit and everything after them
// are StereoBM's.  There is no texture test.
//   1. census_device            both views, all frames -> u64 planes [frame][2][H][W]
//                               (in the buffer the prefilter fills for a SAD call)
//   2. bm_census_match2_kernel  blockSize 5 .. 21, numDisparities <= 128: disparities
//                               on the lanes, decision phase shared with
//                               bm_match2_kernel (mvsv_bm_decide.hpp)
//      bm_census_match_kernel   everything else: 16x16 output tile per block
//   3. bm_finish (mvsv_bm.hip)  validateDisparity, valid rectangle, speckle filter
#include <algorithm>
#include <type_traits>

#include "mvsv_bm_decide.hpp"
#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"

namespace mvsv {
namespace {

using namespace dev;

struct BmcLayout {
    int NJ, NRW, NRC;
    size_t off_r, off_v, off_sad, bytes;
};

__host__ __device__ inline BmcLayout bmc_layout(int nd, int w2, int sad_bytes)
{
    BmcLayout l;
    l.NJ = 16 + 2 * w2;
    l.NRW = 16 + 2 * w2;
    l.NRC = l.NJ + nd;
    l.off_r = (size_t)l.NRW * l.NJ * 8;
    l.off_v = l.off_r + (size_t)l.NRW * l.NRC * 8;
    l.off_sad = l.off_v + (size_t)16 * l.NJ * 4;
    l.bytes = l.off_sad + (size_t)nd * 256 * sad_bytes;
    return l;
}

// bound on the general kernel's global window-sum scratch (per launch)
constexpr size_t kBmcScratchBytes = (size_t)64 << 20;

// The general form: bm_match_kernel's structure (mvsv_bm.hip) on u64 tiles.  T holds
// the descriptors [frame][2][H][W]; gsad / by0 / f0 as there.
template <typename SadT>
__global__ __launch_bounds__(256) void bm_census_match_kernel(const uint64_t* __restrict__ T, int W, int H,
                                                              BmEff e, int keep_border,
                                                              int16_t* __restrict__ out, size_t os, size_t ofs,
                                                              int* __restrict__ cost, SadT* __restrict__ gsad,
                                                              int by0, int f0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nd = e.ndisp, w2 = e.wsz2, win = 2 * w2 + 1;
    const BmcLayout lay = bmc_layout(nd, w2, (int)sizeof(SadT));
    uint64_t* Lt = (uint64_t*)smem;
    uint64_t* Rt = (uint64_t*)(smem + lay.off_r);
    uint32_t* V = (uint32_t*)(smem + lay.off_v);
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    SadT* sadbuf = gsad ? gsad + blk * (size_t)e.ndisp * 256 : (SadT*)(smem + lay.off_sad);
    const int NJ = lay.NJ, NRW = lay.NRW, NRC = lay.NRC;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int f = f0 + (int)blockIdx.z;
    const int xl0 = blockIdx.x * 16;
    const int yr0 = e.ymin + (by0 + (int)blockIdx.y) * 16;
    const int lofs = e.lofs, rofs = e.rofs;
    const size_t plane = (size_t)W * H;
    const uint64_t* Lfr = T + (size_t)f * 2 * plane;
    const uint64_t* Rfr = Lfr + plane;
    const int jmin = xl0 - w2;
    auto clampL = [&](int j) { return lofs + clampi(j, -lofs, W - 1 - lofs); };
    auto clampR = [&](int j) { return clampi(j, -rofs, W - nd - rofs); };
    const int rbase = clampR(jmin);

    // stage the tiles (rows clamped to the image; only valid rows are used)
    for (int i = tid; i < NRW * NJ; i += 256) {
        int r = i / NJ, c = i - r * NJ;
        int yy = clampi(yr0 - w2 + r, 0, H - 1);
        Lt[i] = Lfr[(size_t)yy * W + clampL(jmin + c)];
    }
    for (int i = tid; i < NRW * NRC; i += 256) {
        int r = i / NRC, c = i - r * NRC;
        int yy = clampi(yr0 - w2 + r, 0, H - 1);
        int xx = min(rofs + rbase + c, W - 1);
        Rt[i] = Rfr[(size_t)yy * W + xx];
    }
    __syncthreads();

    const int xl = xl0 + tx, y = yr0 + ty;
    const bool active = xl < e.ncol && y < e.ymax;
    uint32_t minsad = 0xffffffffu;
    int mind = -1;
    for (int k = 0; k < nd; k++) {
        // column sums: thread -> (column c, 4-row chunk)
        for (int item = tid; item < NJ * 4; item += 256) {
            int c = item % NJ, chunk = item / NJ;
            int rc = clampR(jmin + c) - rbase + k;
            int t0 = chunk * 4;
            const uint64_t* lcol = Lt + c;
            const uint64_t* rcol = Rt + rc;
            uint32_t sum = 0;
            for (int r = t0; r < t0 + win; r++) sum += __popcll(lcol[r * NJ] ^ rcol[r * NRC]);
            V[t0 * NJ + c] = sum;
            for (int t = t0 + 1; t < t0 + 4; t++) {
                int ra = t + win - 1, rs = t - 1;
                sum += __popcll(lcol[ra * NJ] ^ rcol[ra * NRC]);
                sum -= __popcll(lcol[rs * NJ] ^ rcol[rs * NRC]);
                V[t * NJ + c] = sum;
            }
        }
        __syncthreads();
        uint32_t sad = 0;
        const uint32_t* vr = V + ty * NJ + tx;
        for (int q = 0; q < win; q++) sad += vr[q];
        sadbuf[k * 256 + tid] = (SadT)sad;
        if (sad < minsad) {
            minsad = sad;
            mind = k;
        }
        __syncthreads();
    }
    if (!active) return;
    const int ximg = lofs + xl;
    int16_t* op = out + f * ofs + (size_t)y * os + ximg;
    if (!keep_border && (ximg < e.xmin || ximg >= e.xmax)) {
        *op = (int16_t)e.filtered;
        return;
    }
    if (e.uniq > 0) {
        const int ms = (int)minsad;
        const int thresh = ms + (ms * e.uniq / 100);
        for (int k = 0; k < nd; k++) {
            if ((k < mind - 1 || k > mind + 1) && (int)sadbuf[k * 256 + tid] <= thresh) {
                *op = (int16_t)e.filtered;
                return;
            }
        }
    }
    const int v1 = nd - mind - 1 + e.mindisp;
    int val;
    if (0 < mind && mind < nd - 1) {
        int p = (int)sadbuf[(mind + 1) * 256 + tid], n = (int)sadbuf[(mind - 1) * 256 + tid];
        int d = p + n - 2 * (int)minsad + abs(p - n);
        val = (v1 * 256 + (d != 0 ? (p - n) * 256 / d : 0) + 15) >> 4;
    } else {
        val = (v1 * 256 + 15) >> 4;
    }
    *op = (int16_t)val;
    if (cost) cost[((size_t)f * H + y) * W + ximg] = (int)minsad;
}

// ---------------------------------------------------------------------------
// bm_census_match2_kernel: disparities on the lanes, bm_match2_kernel's block
// shape.  A 256-thread block stages the left and right descriptors of a
// (64 / NR)-column x TY-row tile plus the window halo in LDS, one dword per
// descriptor for windows of at most 32 bits (WORDS 1), two otherwise; the
// virtual-column clamps are applied while staging the left tile, the right tile
// starts at the clamped column of the tile's first virtual column.  The NR waves
// of a column group hold the disparity indices kk = lane + 64 g:
//   * lane kk reads the right descriptor of column rcol(v) + kk: consecutive lanes
//     read consecutive words (one ds_read_b32 / ds_read_b64); the left descriptor
//     of (row, v) is the same for the whole wave (a broadcast read);
//   * the column sums of popcount(L ^ R) over the window's rows live in registers,
//     one per virtual column, and slide down one row per step: the new row's term
//     is added, the old row's is computed again and subtracted (no ring);
//   * the window sum slides across the virtual columns into the group's
//     [column][disparity] slab; disparity lanes >= numDisparities carry the kPad
//     offset per column sum (21^2 * 64 = 28 224 < 0x10000);
//   * from the slab on: bm2::decide_row, without texture sums.
// ---------------------------------------------------------------------------
struct Bmc2Layout {
    int NJ, NRW, NRC;
    size_t off_r, off_sad, off_rec, bytes;
};

__host__ __device__ inline Bmc2Layout bmc2_layout(int w2, int TY, int NR, int words)
{
    Bmc2Layout l;
    l.NJ = bm2::kWaves / NR * bm2::kCols + 2 * w2;
    l.NRW = TY + 2 * w2;
    l.NRC = l.NJ + 64 * NR;
    l.off_r = ((size_t)l.NRW * l.NJ * 4 * words + 15) & ~(size_t)15;
    l.off_sad = (l.off_r + (size_t)l.NRW * l.NRC * 4 * words + 15) & ~(size_t)15;
    l.off_rec = l.off_sad + (size_t)(bm2::kWaves / NR) * bm2::kCols * (NR * 64 + 4) * 4;
    l.bytes = l.off_rec + (size_t)bm2::kWaves * 64 * 8;
    return l;
}

template <int NR, int W2, int WORDS>
__global__ __launch_bounds__(256) void bm_census_match2_kernel(const uint64_t* __restrict__ T, int W, int H,
                                                               BmEff e, int keep_border, int TY,
                                                               int16_t* __restrict__ out, size_t os, size_t ofs,
                                                               int* __restrict__ cost)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using DescT = std::conditional_t<WORDS == 1, uint32_t, uint64_t>;
    constexpr int win = 2 * W2 + 1;
    constexpr int BC = bm2::kWaves / NR * bm2::kCols;  // output columns per block
    constexpr int NC = bm2::kCols + 2 * W2;            // virtual columns of a column group
    constexpr int NJ = BC + 2 * W2, NRC = NJ + 64 * NR;
    constexpr int SS = NR * 64 + 4;                    // slab column stride (dwords)
    const int nd = e.ndisp;
    const Bmc2Layout lay = bmc2_layout(W2, TY, NR, WORDS);
    const int NRW = lay.NRW;
    DescT* Lt = (DescT*)smem;                 // [NRW][NJ]
    DescT* Rt = (DescT*)(smem + lay.off_r);   // [NRW][NRC]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wv / NR, g = wv % NR;  // column group, disparity block of this wave
    uint32_t* sadx = (uint32_t*)(smem + lay.off_sad) + (size_t)cg * bm2::kCols * SS;
    uint2* recs = (uint2*)(smem + lay.off_rec) + wv * 64;
    const int f = blockIdx.z;
    const int xl0 = blockIdx.x * BC;
    const int yr0 = e.ymin + blockIdx.y * TY;
    const int lofs = e.lofs, rofs = e.rofs;
    const size_t plane = (size_t)W * H;
    const uint64_t* Lfr = T + (size_t)f * 2 * plane;
    const uint64_t* Rfr = Lfr + plane;
    const int jmin = xl0 - W2;
    auto clampR = [&](int j) { return clampi(j, -rofs, W - nd - rofs); };
    const int rbase = clampR(jmin);

    for (int i = tid; i < NRW * NJ; i += 256) {
        const int r = i / NJ, c = i - r * NJ;
        const int yy = clampi(yr0 - W2 + r, 0, H - 1);
        Lt[i] = (DescT)Lfr[(size_t)yy * W + lofs + clampi(jmin + c, -lofs, W - 1 - lofs)];
    }
    for (int i = tid; i < NRW * NRC; i += 256) {
        const int r = i / NRC, c = i - r * NRC;
        const int yy = clampi(yr0 - W2 + r, 0, H - 1);
        Rt[i] = (DescT)Rfr[(size_t)yy * W + min(rofs + rbase + c, W - 1)];
    }

    const int c0 = cg * bm2::kCols;  // the group's first virtual column in the tile
    const int rows = min(TY, e.ymax - yr0);
    // right-tile column of virtual column v: rcol(v) = clampR(jmin + c0 + v) - rbase
    // (wave-uniform).  Groups without a clamp inside their NC columns address it as
    // rcol(0) + v, the others evaluate the clamp per column.
    const int cr0 = clampR(jmin + c0) - rbase;
    const bool lin = clampR(jmin + c0 + NC - 1) - rbase == cr0 + NC - 1;
    const int kl = lane + 64 * g;  // this lane's disparity index
    const uint32_t pad = kl < nd ? 0u : bm2::kPad;
    const bm2::Where where{f, xl0, c0, yr0, W, H, keep_border, out, os, ofs, cost};
    __syncthreads();

    uint32_t cs[NC];
    auto colsums = [&](auto LIN, auto INIT, int t) {
        constexpr bool kLin = decltype(LIN)::value;
        // popcount(L ^ R) of row r, virtual column v, added to acc
        auto term = [&](int r, int v, uint32_t acc) -> uint32_t {
            const int rc = kLin ? cr0 + v : clampR(jmin + c0 + v) - rbase;
            const DescT x = Lt[r * NJ + c0 + v] ^ Rt[r * NRC + rc + kl];
            if constexpr (WORDS == 1)
                return (uint32_t)__builtin_popcount(x) + acc;
            else
                return (uint32_t)__builtin_popcount((uint32_t)(x >> 32)) +
                       ((uint32_t)__builtin_popcount((uint32_t)x) + acc);
        };
        if constexpr (decltype(INIT)::value) {
#pragma unroll
            for (int v = 0; v < NC; v++) cs[v] = pad;
#pragma unroll 1
            for (int r = 0; r < win; r++) {
#pragma unroll
                for (int v = 0; v < NC; v++) cs[v] = term(r, v, cs[v]);
            }
        } else {
            const int rn = t + win - 1, ro = t - 1;
#pragma unroll
            for (int v = 0; v < NC; v++) {
                cs[v] = term(rn, v, cs[v]) - term(ro, v, 0u);
                // bound the LDS loads the scheduler hoists (registers)
                if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // one row's window sums -> slab [column][disparity], then the shared decision
    auto row_out = [&](int t) {
        uint32_t sum = 0;
#pragma unroll
        for (int v = 0; v < win; v++) sum += cs[v];
        sadx[g * 64 + lane] = sum;
#pragma unroll
        for (int x = 1; x < bm2::kCols; x++) {
            sum += cs[x + win - 1];
            sum -= cs[x - 1];
            sadx[x * SS + g * 64 + lane] = sum;
        }
        bm2::decide_row<NR, win, false>(sadx, nullptr, recs, lane, g, t, rows, e, where);
    };
    auto walk = [&](auto LIN) {
        colsums(LIN, std::true_type(), 0);
        row_out(0);
        for (int t = 1; t < rows; t++) {
            colsums(LIN, std::false_type(), t);
            row_out(t);
        }
    };
    if (lin)
        walk(std::true_type());
    else
        walk(std::false_type());
}

typedef void (*Bmc2Fn)(const uint64_t*, int, int, BmEff, int, int, int16_t*, size_t, size_t, int*);

template <int NR, int WORDS>
Bmc2Fn bmc2_pick(int w2)
{
    switch (w2) {
    case 2: return bm_census_match2_kernel<NR, 2, WORDS>;
    case 3: return bm_census_match2_kernel<NR, 3, WORDS>;
    case 4: return bm_census_match2_kernel<NR, 4, WORDS>;
    case 5: return bm_census_match2_kernel<NR, 5, WORDS>;
    case 6: return bm_census_match2_kernel<NR, 6, WORDS>;
    case 7: return bm_census_match2_kernel<NR, 7, WORDS>;
    case 8: return bm_census_match2_kernel<NR, 8, WORDS>;
    case 9: return bm_census_match2_kernel<NR, 9, WORDS>;
    default: return bm_census_match2_kernel<NR, 10, WORDS>;
    }
}

}  // namespace

// The descriptors of both views and the match kernel of a census call (e.cw, e.ch set);
// bm_device has filled the map, handled the empty ranges and ensured `cost`.
int bm_census_match(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs,
                    size_t rfs, int W, int H, const BmEff& e, int16_t* out, size_t os, size_t ofs, int* cost)
{
    hipStream_t s = ctx->stream;
    int rc;
    const size_t plane = (size_t)W * H;
    if ((rc = ensure(ctx, ctx->bm_lf, (size_t)n * 2 * plane * 8, "bm census descriptors"))) return rc;
    uint64_t* T = (uint64_t*)ctx->bm_lf.ptr;
    if ((rc = census_device(ctx, n, 2, L, ls, lfs, R, rs, rfs, W, H, e.cw, e.ch, T, (size_t)W, plane, 2 * plane)))
        return rc;
    const int validate = e.disp12 >= 0 ? 1 : 0;
    const int win = 2 * e.wsz2 + 1, bits = e.cw * e.ch - 1;
    const int nrows = e.ymax - e.ymin;
    if (n > 65535 || (nrows + 3) / 4 > 65535)
        return set_error(ctx, MVSV_E_INVALID_ARG, "census BM: too many frames or rows for one launch");

    if (ctx->opt.bm2 && e.wsz2 >= 2 && e.wsz2 <= 10 && e.ndisp <= 128) {
        const int NR = e.ndisp > 64 ? 2 : 1;
        const int words = bits <= 32 ? 1 : 2;
        const int BC = bm2::kWaves / NR * bm2::kCols;
        const int gx = (e.ncol + BC - 1) / BC;
        const Bmc2Fn kern = NR == 1 ? (words == 1 ? bmc2_pick<1, 1>(e.wsz2) : bmc2_pick<1, 2>(e.wsz2))
                                    : (words == 1 ? bmc2_pick<2, 1>(e.wsz2) : bmc2_pick<2, 2>(e.wsz2));
        // tile height: the rows of a block pay for the window's start-up rows once, a
        // taller tile costs residency.  Take the tallest multiple of 4 up to 32 that
        // keeps two blocks per CU in LDS and still gives every CU two blocks.
        int TY = ctx->opt.bm_ty;
        if (TY <= 0) {
            TY = 4;
            for (int ty = 8; ty <= 32; ty += 4) {
                if (bmc2_layout(e.wsz2, ty, NR, words).bytes > 80 * 1024) break;
                if ((long long)gx * ((nrows + ty - 1) / ty) * n < 2LL * ctx->cus) break;
                TY = ty;
            }
        }
        const Bmc2Layout l2 = bmc2_layout(e.wsz2, TY, NR, words);
        if (l2.bytes > 160 * 1024)
            return set_error(ctx, MVSV_E_INVALID_ARG, "BM tile height too large for LDS");
        if (l2.bytes > 65536 &&
            (rc = check_hip(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)l2.bytes),
                            "bm census LDS attribute")))
            return rc;
        const dim3 grid2(gx, (nrows + TY - 1) / TY, n);
        if (grid2.y > 65535) return set_error(ctx, MVSV_E_INVALID_ARG, "census BM: image too tall for the tile height");
        StageTimer tm(ctx, kStageBm);
        hipLaunchKernelGGL(kern, grid2, dim3(256), l2.bytes, s, (const uint64_t*)T, W, H, e, validate, TY, out, os,
                           ofs, cost);
        return check_hip(ctx, hipGetLastError(), "bm census match");
    }

    const bool small = (long long)win * win * bits <= 65535;
    const BmcLayout lay = bmc_layout(e.ndisp, e.wsz2, small ? 2 : 4);
    const dim3 grid((e.ncol + 15) / 16, (nrows + 15) / 16, n);
    void* gsad = nullptr;
    size_t lds = lay.bytes;
    int rows_per_launch = (int)grid.y;
    if (lay.bytes > 160 * 1024) {
        // window sums in a global scratch slab per block, as bm_device's general form
        lds = lay.off_sad;
        const size_t per_block = (size_t)e.ndisp * 256 * (small ? 2 : 4);
        const size_t per_row = per_block * grid.x;
        rows_per_launch = (int)std::max<size_t>(1, std::min<size_t>(grid.y, kBmcScratchBytes / per_row));
        if ((rc = ensure(ctx, ctx->bm_sad, per_row * rows_per_launch, "bm window-sum scratch"))) return rc;
        gsad = ctx->bm_sad.ptr;
    }
    if (lds > 160 * 1024)
        return set_error(ctx, MVSV_E_INVALID_ARG,
                         "census BM: blockSize and numDisparities too large for the GPU kernel (the descriptor "
                         "tiles do not fit in LDS)");
    if (lds > 65536) {
        const void* fn = small ? (const void*)bm_census_match_kernel<uint16_t>
                               : (const void*)bm_census_match_kernel<uint32_t>;
        if ((rc = check_hip(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                            "bm census LDS attribute")))
            return rc;
    }
    StageTimer tm(ctx, kStageBm);
    auto launch = [&](dim3 g, int by, int f) {
        if (small)
            hipLaunchKernelGGL(bm_census_match_kernel<uint16_t>, g, dim3(256), lds, s, (const uint64_t*)T, W, H, e,
                               validate, out, os, ofs, cost, (uint16_t*)gsad, by, f);
        else
            hipLaunchKernelGGL(bm_census_match_kernel<uint32_t>, g, dim3(256), lds, s, (const uint64_t*)T, W, H, e,
                               validate, out, os, ofs, cost, (uint32_t*)gsad, by, f);
    };
    if (!gsad) {
        launch(grid, 0, 0);
    } else {
        for (int f = 0; f < n; f++)
            for (int by = 0; by < (int)grid.y; by += rows_per_launch)
                launch(dim3(grid.x, std::min(rows_per_launch, (int)grid.y - by), 1), by, f);
    }
    return check_hip(ctx, hipGetLastError(), "bm census match");
}

}  // namespace mvsv
