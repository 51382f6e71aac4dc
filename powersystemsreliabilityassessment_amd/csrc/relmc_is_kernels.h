// relmc_is_kernels.h — kernels of the importance-sampling track (relmc_importance.hip; contract in include/relmc.h): the tilted sampler with
// its likelihood ratios, the weighted scalar sums, and the weighted column sums over a state or nodal matrix.
#pragma once
#include "relmc_devfn.h"

namespace relmc {

constexpr int IS_THREADS = 256;          // workgroup of every kernel here; the sampler stages IS_THREADS state rows in LDS

// relmc_mc_sampling's draws against the tilted thresholds: Philox block blk of sample i = ctr (i_lo, i_hi, blk, 0), key = seed; component
// k = 4 blk + e is down iff word e < thr_is[k] (strict '<', mc_sampling.m:35; the spare words of the last block are ignored).  W needs the
// product over k ascending, so one lane walks one sample's blocks with W in a register: one rounded multiply per component, from 1.0.
// The IS_THREADS rows of a workgroup are contiguous in the row-major matrix: they are staged in LDS (row stride ncomp bytes) and leave as
// one coalesced copy, in 32-bit words when the destination is word-aligned (the tail bytes of a short last tile singly).
// Dynamic LDS: IS_THREADS * ncomp bytes (at most 64 KB at RELMC_MAX_COMP).  eqstatus / weight: either may be null.
__global__ void __launch_bounds__(IS_THREADS) relmc_is_sampling_kernel(const uint32_t* __restrict__ thr_is, const double* __restrict__ r_dn,
                                                                       const double* __restrict__ r_up, int ncomp, uint64_t seed,
                                                                       uint64_t first_index, int64_t n, uint8_t* __restrict__ eqstatus,
                                                                       double* __restrict__ weight)
{
    extern __shared__ uint32_t is_rows_w[];
    uint8_t* const rows = reinterpret_cast<uint8_t*>(is_rows_w);
    const int tid = threadIdx.x, nblk = (ncomp + 3) >> 2;
    for (int64_t base = (int64_t)blockIdx.x * IS_THREADS; base < n; base += (int64_t)gridDim.x * IS_THREADS) {
        const int64_t i = base + tid;
        if (i < n) {
#pragma clang fp contract(off)
            const uint64_t gi = first_index + (uint64_t)i;
            uint8_t* const row = rows + (size_t)tid * ncomp;
            double W = 1.0;
            for (int blk = 0; blk < nblk; ++blk) {
                uint32_t w[4];
                philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)blk, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = blk * 4 + e;
                    if (k < ncomp) {
                        const bool down = w[e] < thr_is[k];
                        W = W * (down ? r_dn[k] : r_up[k]);
                        if (eqstatus) row[k] = down ? 1 : 0;
                    }
                }
            }
            if (weight) weight[i] = W;
        }
        if (eqstatus) {                                              // block-uniform
            __syncthreads();
            const int64_t left = n - base;
            const int bytes = (int)(left < IS_THREADS ? left : IS_THREADS) * ncomp;
            uint8_t* const dst = eqstatus + (size_t)base * ncomp;
            const int words = (reinterpret_cast<uintptr_t>(dst) & 3u) == 0 ? bytes >> 2 : 0;
            for (int j = tid; j < words; j += IS_THREADS) reinterpret_cast<uint32_t*>(dst)[j] = is_rows_w[j];
            for (int j = 4 * words + tid; j < bytes; j += IS_THREADS) dst[j] = rows[j];
            __syncthreads();                                         // the next tile overwrites the rows
        }
    }
}

// Scalar sums of a launch: per sample W, dns (and optionally status, iters) -> per-lane partials over a grid-stride walk, a fixed butterfly
// over the wavefront, the four wavefronts in index order; block b leaves part_d[b][6] = sum W, W^2, W fail, W^2 fail, W dns, (W dns)^2 and
// part_i[b][4] = fail count, singular, non-converged, iterations.  The host adds the blocks in block order (as relmc_hl1_nsq does).  Each
// product is rounded before it is added (no FMA).  f_fail[i] = W fail and f_dns[i] = W dns are the factors of the column sums (may be null).
__global__ void __launch_bounds__(IS_THREADS) relmc_is_scalar_kernel(int64_t n, const double* __restrict__ w, const double* __restrict__ dns,
                                                                     const int32_t* __restrict__ status, const int32_t* __restrict__ iters,
                                                                     double fail_threshold, double* __restrict__ f_fail, double* __restrict__ f_dns,
                                                                     double* __restrict__ part_d, long long* __restrict__ part_i)
{
    __shared__ double red_d[IS_THREADS / 64][6];
    __shared__ long long red_i[IS_THREADS / 64][4];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long c[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * IS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IS_THREADS) {
#pragma clang fp contract(off)
        const double W = w[i], d = dns[i];
        const bool fail = d > fail_threshold;
        const double w2 = W * W, wd = W * d, wf = fail ? W : 0.0;
        s[0] += W; s[1] += w2; s[2] += wf; s[3] += fail ? w2 : 0.0; s[4] += wd; s[5] += wd * wd;
        if (f_fail) f_fail[i] = wf;
        if (f_dns) f_dns[i] = wd;
        c[0] += fail ? 1 : 0;
        if (status) { const int st = status[i]; c[1] += st == 3 ? 1 : 0; c[2] += (st == 1 || st == 2) ? 1 : 0; }
        if (iters) c[3] += iters[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) s[j] += __shfl_xor(s[j], off);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] += __shfl_xor(c[j], off);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) red_d[wv][j] = s[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) red_i[wv][j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x < 6) part_d[(size_t)blockIdx.x * 6 + threadIdx.x] = ((red_d[0][threadIdx.x] + red_d[1][threadIdx.x]) + red_d[2][threadIdx.x]) + red_d[3][threadIdx.x];
    else if (threadIdx.x < 10) { const int j = threadIdx.x - 6; part_i[(size_t)blockIdx.x * 4 + j] = red_i[0][j] + red_i[1][j] + red_i[2][j] + red_i[3][j]; }
}

// Column sums of a row-major matrix rows[n][ncols] (ncols <= IS_THREADS; uint8 states or fp64 nodal values) under a per-sample factor:
// part[b][t] = sum over the samples s of block b's chunk [b chunk, min(n, (b + 1) chunk)), ascending, of factor[s] * rows[s][t], the product
// rounded before it is added.  Lane t owns column t, so the reads of a row are coalesced across the lanes; the factors of IS_THREADS samples at
// a time are staged in LDS and broadcast.  The same kernel serves comp_wfail (factor W fail), comp_wdns (W dns), sum_wnodal (W over the nodal
// matrix) and the tuner's sum e_i x_ik.  The host adds the blocks in block order.
template <class T>
__global__ void __launch_bounds__(IS_THREADS) relmc_is_colsum_kernel(const T* __restrict__ rows, int ncols, const double* __restrict__ factor,
                                                                     int64_t n, int64_t chunk, double* __restrict__ part)
{
    __shared__ double f[IS_THREADS];
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double acc = 0.0;
    for (int64_t s0 = lo; s0 < hi; s0 += IS_THREADS) {
#pragma clang fp contract(off)
        const int m = (int)(hi - s0 < IS_THREADS ? hi - s0 : IS_THREADS);
        __syncthreads();
        if (t < m) f[t] = factor[s0 + t];
        __syncthreads();
        if (t < ncols) {
            const T* const p = rows + (size_t)s0 * ncols + t;
#pragma unroll 4
            for (int j = 0; j < m; ++j) acc += f[j] * (double)p[(size_t)j * ncols];
        }
    }
    if (t < ncols) part[(size_t)blockIdx.x * ncols + t] = acc;
}

}  // namespace relmc
