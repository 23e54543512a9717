// pmx_corr.hip — the binned correlation function: xi(r), xi(r, mu) and multipoles (include/pmesh_amd.h:
// pmx_corr_project, pmx_corr_vjp, pmx_spectral_product; pmesh_amd/correlation.py).
//
// Replaces what a caller of the reference does for it (nbodykit's FFTCorr: a conj(b) as mesh-sized temporaries, c2r,
// then a slab loop of numpy.digitize + bincount over RealField.x).  Three kernels:
//   corr_kernel        the real mesh binned by the separation of its cells, in the tile shape, LDS windows and run sums
//                      of power_kernel (pmx_power.hip), with the helpers of pmx_power_dev.h: one read of the block,
//                      nothing mesh-sized written, no per-cell global atomics
//   corr_vjp_kernel    its adjoint: every cell written once with the coefficients of its bin, gathered from an LDS
//                      window of the coefficient table; the same tiles, windows and bin search, no atomics
//   product_kernel     out = [out +] scale x (conj) y / window, one thread per mode in the memory order of `out`
//                      (PMX_BLOCK_LOOP): the forward product and both products of the gradient
// Every cell has weight 1 (no Hermitian doubling on the real side) and real values: the tables are those of the power
// spectrum without the imaginary columns.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_power_dev.h"

namespace pmx {

// the running sums of one thread for one key (an r bin, or an (r, mu) cell)
template <int N> struct CRun {
    int key;
    double s[N];
    __device__ __forceinline__ void reset(int k)
    {
        key = k;
#pragma unroll
        for (int i = 0; i < N; i++) s[i] = 0;
    }
    __device__ __forceinline__ void flush(double *tab, int stride, int n)
    {
        if (key < 0) return;
        double *t = tab + key * stride;
#pragma unroll
        for (int i = 0; i < N; i++)
            if (i < n) atomicAdd(t + i, s[i]);
    }
};

// what both tile kernels begin with: the tile of this workgroup, its per-axis separations and its range of r bins
struct CTile {
    int64_t o[3];
    int ext[3];
    int blo, bhi;
};

template <bool MU>
__device__ __forceinline__ CTile corr_tile(const PParams &P, const PGeom &g, double *rax, double *smu,
                                           const double *redges, const double *muedges, double (*s_ext)[2],
                                           int *s_range)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    CTile t;
    int64_t tile = blockIdx.x;
    const int c2 = (int)(tile % g.nt[2]);
    tile /= g.nt[2];
    const int c1 = (int)(tile % g.nt[1]), c0 = (int)(tile / g.nt[1]);
    t.o[0] = (int64_t)c0 * PT0;
    t.o[1] = (int64_t)c1 * PT1;
    t.o[2] = (int64_t)c2 * PT2;
    t.ext[0] = (int)min((int64_t)PT0, g.shape[0] - t.o[0]);
    t.ext[1] = (int)min((int64_t)PT1, g.shape[1] - t.o[1]);
    t.ext[2] = (int)min((int64_t)PT2, g.shape[2] - t.o[2]);
    // per-axis separations of the tile and the extreme |r_d| over its index box (waves 0, 1, 2: one axis each)
    // (selects, not t.ext[wv]: an index that is not a constant would put the tile into scratch memory)
    if (wv < 3) {
        const int e = wv == 0 ? t.ext[0] : (wv == 1 ? t.ext[1] : t.ext[2]);
        const int64_t o = wv == 0 ? t.o[0] : (wv == 1 ? t.o[1] : t.o[2]);
        tile_axis_real(g, wv, lane, e, o, rax, s_ext[wv]);
    } else if (MU) {
        for (int i = lane; i <= P.nmu; i += 64) smu[i] = muedges[i];
    }
    __syncthreads();
    if (wv < 2) {
        const int j = tile_bin_range(P, g, wv, lane, s_ext, redges);
        if (lane == 0) s_range[wv] = j;
    }
    __syncthreads();
    t.blo = s_range[0];
    t.bhi = s_range[1];
    return t;
}

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) corr_kernel(PParams P, PGeom g, const char *__restrict__ x,
                                                      const double *__restrict__ redges,
                                                      const double *__restrict__ muedges, double *__restrict__ acc)
{
    extern __shared__ double sm[];
    double *rax = sm;                               // [3][64]  r_d along each memory-order axis of the tile
    double *smu = sm + 2 * PAXIS;                   // nmu + 1  (the layout power_setup sizes: the second table unused)
    double *sed = smu + (MU ? P.nmu + 1 : 0);       // window + 1 r edges
    double *t1 = sed + P.window + 1;                // window * s1
    double *t2 = t1 + P.window * P.s1;              // window * nmu * 4
    __shared__ double s_ext[3][2];
    __shared__ int s_range[2];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CTile t = corr_tile<MU>(P, g, rax, smu, redges, muedges, s_ext, s_range);
    const int blo = t.blo, bhi = t.bhi;
    if (bhi < blo) return;

    const double re0 = redges[0], rinv = P.nk / (redges[P.nk] - redges[0]);
    const double minv = MU ? P.nmu / (smu[P.nmu] - smu[0]) : 0;
    const int nrows = t.ext[0] * t.ext[1];
    const int rper = (nrows + 3) / 4;
    const int r0 = wv * rper, r1 = min(nrows, r0 + rper);
    const bool lane_on = lane < t.ext[2];
    const double r2ax = rax[2 * 64 + lane];
    const int64_t off2 = (t.o[2] + lane) * g.sa[2];
    const int s1 = P.s1, nmu = P.nmu;

    for (int wlo = blo; wlo <= bhi; wlo += P.window) {
        const int nb = min(P.window, bhi - wlo + 1);
        for (int i = tid; i < nb * s1; i += PBLOCK) t1[i] = 0;
        if (MU)
            for (int i = tid; i < nb * nmu * 4; i += PBLOCK) t2[i] = 0;
        for (int i = tid; i <= nb; i += PBLOCK) sed[i] = redges[wlo + i];
        __syncthreads();
        const double wr0 = sed[0], wr1 = sed[nb];

        CRun<POLES ? 3 + PMX_POWER_MAX_POLES : 3> r1d;
        CRun<4> r2d;
        r1d.reset(-1);
        r2d.reset(-1);
        for (int rb = r0; rb < r1; rb += PBATCH) {
            double xv[PBATCH];
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                xv[u] = 0;
                if (r < r1 && lane_on) {
                    const int i0 = r / t.ext[1], i1 = r - i0 * t.ext[1];
                    xv[u] = real_get<T>(x + (t.o[0] + i0) * g.sa[0] + (t.o[1] + i1) * g.sa[1] + off2);
                }
            }
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                if (!(r < r1 && lane_on)) continue;
                const int i0 = r / t.ext[1], i1 = r - i0 * t.ext[1];
                double rr[3];
                const double rmag = mode_k(g, rax[i0], rax[64 + i1], r2ax, rr);
                if (!(rmag >= wr0 && rmag < wr1)) continue;
                const int j = find_bin(sed, nb, rmag, guess(rmag, re0, rinv) - wlo);
                const double v = xv[u] * P.volume;
                double mu = 0;
                if (MU || POLES) mu = mode_mu(g, rr, rmag);

                if (j != r1d.key) {
                    r1d.flush(t1, s1, s1);
                    r1d.reset(j);
                }
                r1d.s[0] += 1.0;
                r1d.s[1] += rmag;
                r1d.s[2] += v;
                if (POLES) {
                    double lp[PMX_POWER_MAX_POLES];
                    legendre_poles(P, mu, lp);
#pragma unroll
                    for (int p = 0; p < PMX_POWER_MAX_POLES; p++) {
                        if (p >= P.npoles) break;
                        r1d.s[3 + p] += v * lp[p];
                    }
                }
                if (MU) {
                    const int m = mu_bin(smu, nmu, mu, minv);
                    if (m >= 0) {
                        const int c = j * nmu + m;
                        if (c != r2d.key) { r2d.flush(t2, 4, 4); r2d.reset(c); }
                        r2d.s[0] += 1.0;
                        r2d.s[1] += rmag;
                        r2d.s[2] += mu;
                        r2d.s[3] += v;
                    }
                }
            }
        }
        r1d.flush(t1, s1, s1);
        if (MU) r2d.flush(t2, 4, 4);
        __syncthreads();
        // the window into the global sums: contiguous runs of doubles, bins that received nothing skipped
        double *g1 = acc + (int64_t)wlo * s1;
        for (int i = tid; i < nb * s1; i += PBLOCK)
            if (t1[(i / s1) * s1] != 0) unsafeAtomicAdd(g1 + i, t1[i]);
        if (MU) {
            double *g2 = acc + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 4;
            for (int i = tid; i < nb * nmu * 4; i += PBLOCK)
                if (t2[(i / 4) * 4] != 0) unsafeAtomicAdd(g2 + i, t2[i]);
        }
        __syncthreads();
    }
}

// A tile that spans more bins than a window holds takes one pass per window, and each of its cells is written by
// exactly one pass: the pass whose window holds its bin, or the first one (zero) when it has no bin.
template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) corr_vjp_kernel(PParams P, PGeom g, char *__restrict__ out,
                                                          const double *__restrict__ redges,
                                                          const double *__restrict__ muedges,
                                                          const double *__restrict__ coef)
{
    extern __shared__ double sm[];
    double *rax = sm;
    double *smu = sm + 2 * PAXIS;
    double *sed = smu + (MU ? P.nmu + 1 : 0);
    double *t1 = sed + P.window + 1;                // window * s1 coefficients of the r bins
    double *t2 = t1 + P.window * P.s1;              // window * nmu coefficients of the (r, mu) cells
    __shared__ double s_ext[3][2];
    __shared__ int s_range[2];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CTile t = corr_tile<MU>(P, g, rax, smu, redges, muedges, s_ext, s_range);
    const int blo = t.blo, bhi = t.bhi;

    const int nrows = t.ext[0] * t.ext[1];
    const int rper = (nrows + 3) / 4;
    const int r0 = wv * rper, r1 = min(nrows, r0 + rper);
    const bool lane_on = lane < t.ext[2];
    const int64_t off2 = (t.o[2] + lane) * g.sa[2];

    if (bhi < blo) {
        // no cell of the tile has an r bin: zeros
        if (lane_on)
            for (int r = r0; r < r1; r++) {
                const int i0 = r / t.ext[1], i1 = r - i0 * t.ext[1];
                real_put<T>(out + (t.o[0] + i0) * g.sa[0] + (t.o[1] + i1) * g.sa[1] + off2, 0.0);
            }
        return;
    }

    const double re0 = redges[0], rinv = P.nk / (redges[P.nk] - redges[0]);
    const double rlo = redges[blo], rhi = redges[bhi + 1];     // the tile's passes cover [rlo, rhi)
    const double minv = MU ? P.nmu / (smu[P.nmu] - smu[0]) : 0;
    const double r2ax = rax[2 * 64 + lane];
    const int s1 = P.s1, nmu = P.nmu;

    for (int wlo = blo; wlo <= bhi; wlo += P.window) {
        const int nb = min(P.window, bhi - wlo + 1);
        const double *g1 = coef + (int64_t)wlo * s1;
        for (int i = tid; i < nb * s1; i += PBLOCK) t1[i] = g1[i];
        if (MU) {
            const double *g2 = coef + (int64_t)P.nk * s1 + (int64_t)wlo * nmu;
            for (int i = tid; i < nb * nmu; i += PBLOCK) t2[i] = g2[i];
        }
        for (int i = tid; i <= nb; i += PBLOCK) sed[i] = redges[wlo + i];
        __syncthreads();
        const double wr0 = sed[0], wr1 = sed[nb];
        const bool first = wlo == blo;

        if (lane_on)
            for (int r = r0; r < r1; r++) {
                const int i0 = r / t.ext[1], i1 = r - i0 * t.ext[1];
                double rr[3];
                const double rmag = mode_k(g, rax[i0], rax[64 + i1], r2ax, rr);
                double f = 0;
                if (rmag >= wr0 && rmag < wr1) {
                    const int j = find_bin(sed, nb, rmag, guess(rmag, re0, rinv) - wlo);
                    double mu = 0;
                    if (MU || POLES) mu = mode_mu(g, rr, rmag);
                    const double *c = t1 + j * s1;
                    f = c[0];
                    if (POLES) {
                        double lp[PMX_POWER_MAX_POLES];
                        legendre_poles(P, mu, lp);
#pragma unroll
                        for (int p = 0; p < PMX_POWER_MAX_POLES; p++) {
                            if (p >= P.npoles) break;
                            f += lp[p] * c[1 + p];
                        }
                    }
                    if (MU) {
                        const int m = mu_bin(smu, nmu, mu, minv);
                        if (m >= 0) f += t2[j * nmu + m];
                    }
                    f *= P.volume;
                } else if (!(first && !(rmag >= rlo && rmag < rhi))) {
                    continue;                       // another pass holds the bin of this cell
                }
                real_put<T>(out + (t.o[0] + i0) * g.sa[0] + (t.o[1] + i1) * g.sa[1] + off2, f);
            }
        __syncthreads();
    }
}

// out = (ACC ? out : 0) + scale x (CONJ ? conj(y) : y) / prod_d sinc(w_d / 2)^deconv_pow
template <typename T, bool CONJ, bool ACC, bool WIN>
__global__ void __launch_bounds__(256) product_kernel(double scale, int deconv_pow, BlockGeom g, const char *x,
                                                      BlockStr xs, const char *y, BlockStr ys, char *out, BlockStr os)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double xr, xi, yr, yi;
        CLoad<T>::get(x + xs.off(idx), xr, xi);
        CLoad<T>::get(y + ys.off(idx), yr, yi);
        if (CONJ) yi = -yi;
        double pr = scale * (xr * yr - xi * yi), pi = scale * (xr * yi + xi * yr);
        if (WIN) {
            double comp = 1;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                if (d >= g.ndim) break;
                comp *= sinc_pow(mode_w(idx[d] + g.start[d], g.nmesh[d], g.dw[d]), deconv_pow);
            }
            pr /= comp;
            pi /= comp;
        }
        char *p = out + os.off(idx);
        if (ACC) {
            double ar, ai;
            CLoad<T>::get(p, ar, ai);
            pr += ar;
            pi += ai;
        }
        CLoad<T>::put(p, pr, pi);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

// the arguments both tile entries share, checked, and the kernel parameters (per_bin / per_cell doubles per r bin /
// (r, mu) cell of the table whose window lives in LDS)
static int corr_setup(const pmx_power *p, int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides,
                      const int64_t *shape, const int64_t *start, const int64_t *nmesh, const double *boxsize,
                      const double *redges, const double *muedges, int per_bin, int per_cell, PParams &P, PGeom &g,
                      int64_t *ntiles, size_t *lds)
{
    PMX_REQUIRE(p, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(p->hermitian == 0 && p->deconv_pow == 0, PMX_EINVAL, "hermitian and deconv_pow must be 0 on the real side");
    for (int d = 0; d < ndim && d < 3 && boxsize; d++)
        PMX_REQUIRE(boxsize[d] > 0 && isfinite(boxsize[d]), PMX_EINVAL, "bad boxsize");
    return power_setup(p, ndim, elsize, x, x_strides, nullptr, nullptr, shape, start, nmesh, boxsize, redges, muedges,
                       per_bin, per_cell, P, g, ntiles, lds);
}

extern "C" int pmx_corr_project(const pmx_power *p, int32_t ndim, int32_t elsize, const void *x,
                                const int64_t *x_strides, const int64_t *shape, const int64_t *start,
                                const int64_t *nmesh, const double *boxsize, const double *redges,
                                const double *muedges, double *acc, void *stream)
{
    PMX_REQUIRE(acc, PMX_EINVAL, "bad arguments");
    PParams P;
    PGeom g;
    int64_t ntiles;
    size_t lds = 0;
    const int rc = corr_setup(p, ndim, elsize, x, x_strides, shape, start, nmesh, boxsize, redges, muedges,
                              3 + (p ? p->npoles : 0), 4, P, g, &ntiles, &lds);
    if (rc != PMX_OK || ntiles == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ntiles);
    const bool mu = p->nmu > 0, poles = p->npoles > 0;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mu, [&](auto m) {
            with_bool(poles, [&](auto pl) {
                corr_kernel<T, m, pl><<<grid, PBLOCK, lds, s>>>(P, g, (const char *)x, redges, muedges, acc);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_corr_vjp(const pmx_power *p, int32_t ndim, int32_t elsize, void *gr, const int64_t *g_strides,
                            const int64_t *shape, const int64_t *start, const int64_t *nmesh, const double *boxsize,
                            const double *redges, const double *muedges, const double *coef, void *stream)
{
    PMX_REQUIRE(coef, PMX_EINVAL, "bad arguments");
    PParams P;
    PGeom g;
    int64_t ntiles;
    size_t lds = 0;
    const int rc = corr_setup(p, ndim, elsize, gr, g_strides, shape, start, nmesh, boxsize, redges, muedges,
                              1 + (p ? p->npoles : 0), 1, P, g, &ntiles, &lds);
    if (rc != PMX_OK || ntiles == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ntiles);
    const bool mu = p->nmu > 0, poles = p->npoles > 0;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mu, [&](auto m) {
            with_bool(poles, [&](auto pl) {
                corr_vjp_kernel<T, m, pl><<<grid, PBLOCK, lds, s>>>(P, g, (char *)gr, redges, muedges, coef);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

// the bytes [lo, hi) a strided block of complex elements of 2 * elsize bytes reaches
static void product_span(const void *base, const BlockGeom &g, const BlockStr &s, int elsize, intptr_t &lo, intptr_t &hi)
{
    lo = hi = (intptr_t)base;
    for (int d = 0; d < 3; d++) {
        const int64_t reach = (g.shape[d] - 1) * s.s[d];
        if (reach < 0) lo += reach;
        else hi += reach;
    }
    hi += 2 * elsize;
}

// out may be the input itself, element for element (the same pointer and the same strides on every axis longer than
// one), or must not reach its bytes
static bool product_alias_ok(const void *in, const BlockStr &is, const void *out, const BlockStr &os, const BlockGeom &g,
                             int elsize)
{
    if (in == out) {
        for (int d = 0; d < 3; d++)
            if (g.shape[d] > 1 && is.s[d] != os.s[d]) return false;
        return true;
    }
    intptr_t ilo, ihi, olo, ohi;
    product_span(in, g, is, elsize, ilo, ihi);
    product_span(out, g, os, elsize, olo, ohi);
    return ihi <= olo || ohi <= ilo;
}

extern "C" int pmx_spectral_product(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides,
                                    const void *y, const int64_t *y_strides, void *out, const int64_t *out_strides,
                                    const int64_t *shape, const int64_t *start, const int64_t *nmesh, double scale,
                                    int32_t conj_y, int32_t accumulate, int32_t deconv_pow, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    PMX_REQUIRE(x && x_strides && y && y_strides && out && out_strides && shape && start && nmesh, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(deconv_pow >= 0, PMX_EINVAL, "deconv_pow must not be negative");
    for (int d = 0; d < ndim; d++) PMX_REQUIRE(shape[d] >= 0 && nmesh[d] >= 1, PMX_EINVAL, "bad geometry");
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, nullptr, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr xs = make_str(ndim, x_strides), ys = make_str(ndim, y_strides), os = make_str(ndim, out_strides);
    PMX_REQUIRE(product_alias_ok(x, xs, out, os, g, elsize), PMX_EINVAL, "out overlaps x without being x");
    PMX_REQUIRE(product_alias_ok(y, ys, out, os, g, elsize), PMX_EINVAL, "out overlaps y without being y");
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(conj_y != 0, [&](auto cj) {
            with_bool(accumulate != 0, [&](auto ac) {
                with_bool(deconv_pow != 0, [&](auto wn) {
                    product_kernel<T, cj, ac, wn><<<grid, 256, 0, st>>>(scale, deconv_pow, g, (const char *)x, xs,
                                                                        (const char *)y, ys, (char *)out, os);
                });
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
