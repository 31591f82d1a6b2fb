// mvsv_tm.hip — Disparity::tm (src/disparity.cpp:25-58) on MI355X: for every pixel
// (i, j) with i < H - k, j < W - k the k x k template L[i.., j..] is matched against
// the windows R[i.., j + x ..], x = 0 .. W - j - k - 1, by cv::matchTemplate(...,
// CV_TM_CCORR_NORMED) and the first x with the largest score is stored.  The score
// N / sqrt(sum T^2 * sum S^2), N = sum T * S, is compared in exact integers: x beats
// the best b so far iff N_x^2 * SS_b > N_b^2 * SS_x (sum T^2 is common to a pixel's
// candidates), strictly, so the earliest x keeps a tie; a window of zeros (or a zero
// template) scores 0.  DESIGN.md §4n.
//
// One block: one image row i, kTmJT = 256 template columns, every shift, in chunks of
// kTmXC = 32 shifts.  Per chunk
//   stage   the k rows of R under the chunk, four rows per dword (rows past k are 0),
//           into LDS; L's columns are staged once per block
//   squares CS[col] = sum over the k rows of R^2 (v_dot4_u32_u8 of a dword with itself),
//           then SS[r] = sum of k consecutive CS
//   phase 1 thread = (shift, group of 32 columns): the column products
//           V(c) = sum over rows of L(c) * R(c + x) are ceil(k / 4) v_dot4_u32_u8; the
//           window sum N slides along j (N += V(j + k) - V(j)), so a candidate costs two
//           V whatever k is; N goes into a 256 x 32 LDS tile (pitch 33)
//   phase 2 thread = column j: walks the tile's 32 shifts in order with its running
//           best (N, SS, x) in registers.  A float product filter (relative error far
//           below its 2^-18 slack) drops candidates that cannot win; every candidate
//           that might is decided by the 128-bit integer comparison.
// The kernel is instantiated for Q = ceil(k / 4) = 1 .. 8, so the dot-product loops
// unroll and the LDS row strides are constants.
// The work per column is triangular (W - j - k shifts); blocks with the smallest j are
// the longest and come first in blockIdx.x.  No block waits for another; every loop is
// bounded by W.
#include "mvsv_device.hpp"
#include "mvsv_internal.hpp"
#include "mvsv_stage.hpp"

namespace mvsv {
namespace {

constexpr int kTmJT = 256;            // template columns per block (= threads)
constexpr int kTmXC = 32;             // shifts per chunk
constexpr int kTmPitch = kTmXC + 1;   // tile row pitch in dwords: column j's reads hit 32 banks
constexpr int kTmMaxK = 31;

// rows 4q .. 4q+3 of column `col` below `row0` as one dword; rows >= k and columns >= W are 0
__device__ __forceinline__ uint32_t tm_pack(const uint8_t* __restrict__ row0, size_t stride, int col, int W, int q,
                                            int k)
{
    uint32_t v = 0;
    if (col < W) {
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (4 * q + b < k) v |= (uint32_t)row0[(size_t)(4 * q + b) * stride + col] << (8 * b);
    }
    return v;
}

// N^2 * SSb > Nb^2 * SS in 128 bits (N < 2^26, SS < 2^26: products below 2^78)
__device__ __forceinline__ bool tm_beats(uint32_t N, uint32_t SS, uint32_t Nb, uint32_t SSb)
{
    const unsigned __int128 a = (unsigned __int128)((uint64_t)N * N) * SSb;
    const unsigned __int128 b = (unsigned __int128)((uint64_t)Nb * Nb) * SS;
    return a > b;
}

// LDS row strides for a kernel built for k <= 4 * Q: every index below stays inside
constexpr int tm_lw(int Q) { return kTmJT - 1 + 4 * Q; }          // Lp: local columns <= 254 + k
constexpr int tm_rw(int Q) { return kTmJT + kTmXC - 1 + 4 * Q; }  // Rp, CS: <= 285 + k
constexpr int kTmSS = kTmJT + kTmXC - 1;                          // SSr: <= 286
constexpr int tm_lds_dwords(int Q) { return Q * tm_lw(Q) + Q * tm_rw(Q) + tm_rw(Q) + kTmSS + kTmJT * kTmPitch; }

// V(c) at shift xx: the products of L's column c and R's column c + xx over the k rows
template <int Q>
__device__ __forceinline__ uint32_t tm_colprod(const uint32_t* Lp, const uint32_t* Rp, int c, int xx)
{
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) s = __builtin_amdgcn_udot4(Lp[q * tm_lw(Q) + c], Rp[q * tm_rw(Q) + c + xx], s, false);
    return s;
}

// U steps of the sliding window sum from local column c (the window that starts at c):
// all 2 * U column products are read before the first N is stored
template <int Q, int U>
__device__ __forceinline__ void tm_slide(const uint32_t* Lp, const uint32_t* Rp, uint32_t* tile, int c, int k, int xx,
                                         uint32_t& N)
{
    uint32_t in[U], gone[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        in[u] = tm_colprod<Q>(Lp, Rp, c + u + k - 1, xx);
        gone[u] = tm_colprod<Q>(Lp, Rp, c + u - 1, xx);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        N += in[u] - gone[u];
        tile[(c + u) * kTmPitch + xx] = N;
    }
}

// Q = ceil(k / 4): the dwords of a packed column
template <typename OutT, int Q>
__global__ __launch_bounds__(kTmJT) void tm_kernel(const uint8_t* __restrict__ left, size_t ls, size_t lfs,
                                                   const uint8_t* __restrict__ right, size_t rs, size_t rfs, int W,
                                                   int H, int k, uint8_t* __restrict__ dst, size_t ds, size_t dfs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tm_lds[];
    constexpr int LW = tm_lw(Q), RW = tm_rw(Q);
    const int t = threadIdx.x, j0 = blockIdx.x * kTmJT, i = blockIdx.y, j = j0 + t;
    const size_t f = blockIdx.z;
    OutT* out = reinterpret_cast<OutT*>(dst + f * dfs + (size_t)i * ds);
    if (i >= H - k) {  // the same for the whole block
        if (j < W) out[j] = 0;
        return;
    }
    uint32_t* Lp = tm_lds;                  // [Q][LW]  L columns j0 ..
    uint32_t* Rp = Lp + Q * LW;             // [Q][RW]  R columns j0 + xb ..
    uint32_t* CS = Rp + Q * RW;             // [RW]     column sums of R^2
    uint32_t* SSr = CS + RW;                // [kTmSS]  window sums of R^2
    uint32_t* tile = SSr + kTmSS;           // [kTmJT][kTmPitch] N of (column, shift in chunk)
    const uint8_t* Lrow = left + f * lfs + (size_t)i * ls;
    const uint8_t* Rrow = right + f * rfs + (size_t)i * rs;
    const int nx0 = W - j0 - k;  // shifts of the block's first column
    const int nx = W - j - k;    // shifts of this thread's column (<= 0: none)
    if (nx0 > 0)
        for (int e = t; e < Q * LW; e += kTmJT) {
            const int q = e / LW, col = e - q * LW;
            Lp[e] = tm_pack(Lrow, ls, j0 + col, W, q, k);
        }
    uint32_t bN = 0, bS = 1, bx = 0;  // best so far: a score of 0 at x = 0
    float bN2f = 0.f, bSf = 1.f;
    const float slack = 1.0f + 1.0f / 262144.0f;
    const int xx = t & (kTmXC - 1), c0 = (t >> 5) * 32;
    for (int xb = 0; xb < nx0; xb += kTmXC) {
        const int rb = j0 + xb;
        for (int e = t; e < Q * RW; e += kTmJT) {
            const int q = e / RW, col = e - q * RW;
            Rp[e] = tm_pack(Rrow, rs, rb + col, W, q, k);
        }
        __syncthreads();
        for (int col = t; col < RW; col += kTmJT) {
            uint32_t s = 0;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const uint32_t v = Rp[q * RW + col];
                s = __builtin_amdgcn_udot4(v, v, s, false);
            }
            CS[col] = s;
        }
        __syncthreads();
        for (int r = t; r < kTmSS; r += kTmJT) {
            uint32_t s = 0;
            for (int c = 0; c < k; c++) s += CS[r + c];
            SSr[r] = s;
        }
        {
            // phase 1: shift xb + xx, local columns c0 .. c0 + 31.  Indices stay inside Lp / Rp
            // for every thread, so candidates past the image are computed and never read
            uint32_t N = 0;
            for (int c = 0; c < k; c++) N += tm_colprod<Q>(Lp, Rp, c0 + c, xx);
            tile[c0 * kTmPitch + xx] = N;
            for (int s = 1; s < 29; s += 4) tm_slide<Q, 4>(Lp, Rp, tile, c0 + s, k, xx, N);
            tm_slide<Q, 3>(Lp, Rp, tile, c0 + 29, k, xx, N);
        }
        __syncthreads();
        // phase 2: this column's shifts of the chunk in order, eight loaded at a time
        const int m = nx - xb;
        for (int x2 = 0; x2 < kTmXC && x2 < m; x2 += 8) {
            uint32_t Nn[8], Ss[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                Nn[u] = tile[t * kTmPitch + x2 + u];
                Ss[u] = SSr[t + x2 + u];  // > 0 wherever N > 0
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t N = x2 + u < m ? Nn[u] : 0u, S = Ss[u];
                const float Nf = (float)N, Sf = (float)S;
                const float N2f = Nf * Nf;
                if (N != 0 && N2f * bSf * slack >= bN2f * Sf && tm_beats(N, S, bN, bS)) {
                    bN = N;
                    bS = S;
                    bx = (uint32_t)(xb + x2 + u);
                    bN2f = N2f;
                    bSf = Sf;
                }
            }
        }
        // the next chunk writes Rp, then CS, then SSr / tile, each behind a barrier of its own
    }
    if (j < W) out[j] = nx > 0 ? (OutT)bx : (OutT)0;
}

template <typename OutT>
void tm_launch(int Q, dim3 grid, hipStream_t stream, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R,
               size_t rs, size_t rfs, int W, int H, int k, uint8_t* dst, size_t ds, size_t dfs)
{
#define MVSV_TM_CASE(q)                                                                                              \
    case q:                                                                                                          \
        hipLaunchKernelGGL((tm_kernel<OutT, q>), grid, dim3(kTmJT), sizeof(uint32_t) * tm_lds_dwords(q), stream, L,  \
                           ls, lfs, R, rs, rfs, W, H, k, dst, ds, dfs);                                              \
        break;
    switch (Q) {
        MVSV_TM_CASE(1)
        MVSV_TM_CASE(2)
        MVSV_TM_CASE(3)
        MVSV_TM_CASE(4)
        MVSV_TM_CASE(5)
        MVSV_TM_CASE(6)
        MVSV_TM_CASE(7)
        MVSV_TM_CASE(8)
    }
#undef MVSV_TM_CASE
}

}  // namespace

int tm_validate(int k, int W, int H, std::string* why)
{
    auto bad = [&](const char* m) {
        if (why) *why = m;
        return (int)MVSV_E_INVALID_ARG;
    };
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return bad("tm: image size must be within 1 .. 65535");
    if (k < 1 || k > kTmMaxK) return bad("tm: kernelSize must be within 1 .. 31");
    if (k >= std::min(W, H)) return bad("tm: kernelSize must be smaller than both image sides");
    return MVSV_OK;
}

int tm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs, size_t rfs,
              int W, int H, int k, void* dst, size_t ds, size_t dfs, int elem_bytes)
{
    std::string why;
    if (tm_validate(k, W, H, &why)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    if (elem_bytes != 1 && elem_bytes != 2) return set_error(ctx, MVSV_E_INVALID_ARG, "tm: elem_bytes must be 1 or 2");
    if (n < 1 || n > 65535) return set_error(ctx, MVSV_E_INVALID_ARG, "tm: batch must be within 1 .. 65535");
    if (ls < (size_t)W || rs < (size_t)W || ds < (size_t)W * elem_bytes)
        return set_error(ctx, MVSV_E_INVALID_ARG, "tm: stride smaller than the row");
    if (n == 1) lfs = rfs = dfs = 0;
    if (elem_bytes == 2 && (((uintptr_t)dst | ds | dfs) & 1))
        return set_error(ctx, MVSV_E_INVALID_ARG, "tm: a 16-bit destination needs an even base and even strides");
    dim3 grid((W + kTmJT - 1) / kTmJT, H, n);
    const int Q = (k + 3) >> 2;  // 1 .. 8
    if (elem_bytes == 1)
        tm_launch<uint8_t>(Q, grid, ctx->stream, L, ls, lfs, R, rs, rfs, W, H, k, (uint8_t*)dst, ds, dfs);
    else
        tm_launch<uint16_t>(Q, grid, ctx->stream, L, ls, lfs, R, rs, rfs, W, H, k, (uint8_t*)dst, ds, dfs);
    return check_hip(ctx, hipGetLastError(), "tm");
}

}  // namespace mvsv

using namespace mvsv;

extern "C" {

int mvsv_tm_validate(int k, int W, int H) { return tm_validate(k, W, H, nullptr); }

// [Disparity::tm] src/disparity.cpp:25-58
int mvsv_tm_device(mvsv_ctx* ctx, int n, const uint8_t* L, size_t ls, size_t lfs, const uint8_t* R, size_t rs,
                   size_t rfs, int W, int H, int k, void* dst, size_t ds, size_t dfs, int elem_bytes)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    if (!L || !R || !dst) return set_error(ctx, MVSV_E_INVALID_ARG, "tm: null image");
    DeviceGuard dev_guard(ctx->device);
    return mark_last_use(ctx, tm_device(ctx, n, L, ls, lfs, R, rs, rfs, W, H, k, dst, ds, dfs, elem_bytes));
}

int mvsv_tm(mvsv_ctx* ctx, const uint8_t* L, size_t ls, const uint8_t* R, size_t rs, int W, int H, int k,
            uint8_t* dst, size_t ds)
{
    if (!ctx) return MVSV_E_INVALID_ARG;
    std::string why;
    if (!L || !R || !dst) return set_error(ctx, MVSV_E_INVALID_ARG, "tm: null image");
    if (tm_validate(k, W, H, &why)) return set_error(ctx, MVSV_E_INVALID_ARG, why);
    if (ls < (size_t)W || rs < (size_t)W || ds < (size_t)W)
        return set_error(ctx, MVSV_E_INVALID_ARG, "tm: stride smaller than the row");
    DeviceGuard dev_guard(ctx->device);
    const PairStage s(W, H, 1, 1);
    return staged_call(ctx, s, "tm staging", [&](Staging& sg) -> int {
        int rc;
        uint8_t* dl = sg.at<uint8_t>(s.left);
        uint8_t* dr = sg.at<uint8_t>(s.right);
        uint8_t* dout = sg.at<uint8_t>(s.out);
        if ((rc = sg.up(dl, W, L, ls, W, H, "H2D image")) || (rc = sg.up(dr, W, R, rs, W, H, "H2D image")) ||
            (rc = tm_device(ctx, 1, dl, W, s.left.bytes, dr, W, s.right.bytes, W, H, k, dout, W, s.out.bytes, 1)) ||
            (rc = sg.down(dst, ds, dout, W, W, H, "D2H image")))
            return rc;
        return sg.finish();
    });
}

}  // extern "C"
