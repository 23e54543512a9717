// pmx_corr.hip — the binned correlation function: xi(r), xi(r, mu) and multipoles (include/pmesh_amd.h:
// pmx_corr_project, pmx_corr_vjp, pmx_spectral_product; pmesh_amd/correlation.py).
//
// Replaces what a caller of the reference does for it (nbodykit's FFTCorr: a conj(b) as mesh-sized temporaries, c2r,
// then a slab loop of numpy.digitize + bincount over RealField.x).  Three kernels:
//   corr_kernel        the real mesh binned by the separation of its cells: power_kernel (pmx_power.hip) on the real
//                      side, in the same skeleton of pmx_power_dev.h (tile_begin<true, MU>, the row split, the window
//                      loop, Run): one read of the block, nothing mesh-sized written, no per-cell global atomics
//   corr_vjp_kernel    its adjoint: every cell written once with the coefficients of its bin, gathered from an LDS
//                      window of the coefficient table; the same skeleton (each cell written by exactly one pass:
//                      the rule of pass_writes_zero; tile_zero), no atomics
//   product_kernel     out = [out +] scale x (conj) y / window, one thread per mode in the memory order of `out`
//                      (PMX_BLOCK_LOOP): the forward product and both products of the gradient
// Every cell has weight 1 (no Hermitian doubling on the real side) and real values: the tables are those of the power
// spectrum without the imaginary columns.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_power_dev.h"

namespace pmx {

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) corr_kernel(PParams P, PGeom g, const char *__restrict__ x,
                                                      const double *__restrict__ redges,
                                                      const double *__restrict__ muedges, double *__restrict__ acc)
{
    extern __shared__ double sm[];
    const PLds L = lds_layout<MU>(sm, P);           // kax: r_d; t1: window * s1 sums, t2: window * nmu * 4
    const PTile t = tile_begin<true, MU>(P, g, L, redges, muedges);
    if (t.bhi < t.blo) return;

    const PGuess q = bin_guess<MU>(P, L, redges);
    const PRows w = wave_rows(t);
    const double r2ax = L.kax[2 * 64 + (threadIdx.x & 63)];
    const int64_t off2 = lane_off(t, g.sa);
    const int s1 = P.s1, nmu = P.nmu;

    for (int wlo = t.blo; wlo <= t.bhi; wlo += P.window) {
        const int nb = window_edges(P, t, wlo, L.sed, redges);
        window_zero(L.t1, nb * s1);
        if (MU) window_zero(L.t2, nb * nmu * 4);
        __syncthreads();
        const double wr0 = L.sed[0], wr1 = L.sed[nb];

        Run<POLES ? 3 + PMX_POWER_MAX_POLES : 3> r1d;
        Run<4> r2d;
        r1d.reset(-1);
        r2d.reset(-1);
        for (int rb = w.r0; rb < w.r1; rb += PBATCH) {
            double xv[PBATCH];
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                xv[u] = 0;
                if (r < w.r1 && w.lane_on) {
                    int i0, i1;
                    row_index(t, r, i0, i1);
                    xv[u] = real_get<T>(row_ptr(x, t, g.sa, i0, i1, off2));
                }
            }
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                if (!(r < w.r1 && w.lane_on)) continue;
                int i0, i1;
                row_index(t, r, i0, i1);
                double rr[3];
                const double rmag = mode_k(g, L.kax[i0], L.kax[64 + i1], r2ax, rr);
                if (!(rmag >= wr0 && rmag < wr1)) continue;
                const int j = window_bin(L.sed, nb, wlo, rmag, q);
                const double v = xv[u] * P.volume;
                double mu = 0;
                if (MU || POLES) mu = mode_mu(g, rr, rmag);

                r1d.select(j, L.t1, s1);
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
                    const int m = mu_bin(L.smu, nmu, mu, q.minv);
                    if (m >= 0) {
                        r2d.select(j * nmu + m, L.t2, 4);
                        r2d.s[0] += 1.0;
                        r2d.s[1] += rmag;
                        r2d.s[2] += mu;
                        r2d.s[3] += v;
                    }
                }
            }
        }
        r1d.flush(L.t1, s1, s1);
        if (MU) r2d.flush(L.t2, 4, 4);
        __syncthreads();
        window_add(acc + (int64_t)wlo * s1, L.t1, nb * s1, s1);
        if (MU) window_add(acc + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 4, L.t2, nb * nmu * 4, 4);
        __syncthreads();
    }
}

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) corr_vjp_kernel(PParams P, PGeom g, char *__restrict__ out,
                                                          const double *__restrict__ redges,
                                                          const double *__restrict__ muedges,
                                                          const double *__restrict__ coef)
{
    extern __shared__ double sm[];
    const PLds L = lds_layout<MU>(sm, P);           // kax: r_d; t1: window * s1 coefficients, t2: window * nmu
    const PTile t = tile_begin<true, MU>(P, g, L, redges, muedges);

    const PRows w = wave_rows(t);
    const int64_t off2 = lane_off(t, g.sa);
    auto put = [&](int i0, int i1, double f) { real_put<T>(row_ptr(out, t, g.sa, i0, i1, off2), f); };
    if (t.bhi < t.blo) {
        tile_zero(t, w, [&](int i0, int i1) { put(i0, i1, 0.0); });
        return;
    }

    const PGuess q = bin_guess<MU>(P, L, redges);
    const double rlo = redges[t.blo], rhi = redges[t.bhi + 1];     // the tile's passes cover [rlo, rhi)
    const double r2ax = L.kax[2 * 64 + (threadIdx.x & 63)];
    const int s1 = P.s1, nmu = P.nmu;

    for (int wlo = t.blo; wlo <= t.bhi; wlo += P.window) {
        const int nb = window_edges(P, t, wlo, L.sed, redges);
        window_load(L.t1, nb * s1, coef + (int64_t)wlo * s1);
        if (MU) window_load(L.t2, nb * nmu, coef + (int64_t)P.nk * s1 + (int64_t)wlo * nmu);
        __syncthreads();
        const double wr0 = L.sed[0], wr1 = L.sed[nb];
        const bool first = wlo == t.blo;

        if (w.lane_on)
            for (int r = w.r0; r < w.r1; r++) {
                int i0, i1;
                row_index(t, r, i0, i1);
                double rr[3];
                const double rmag = mode_k(g, L.kax[i0], L.kax[64 + i1], r2ax, rr);
                double f = 0;
                if (rmag >= wr0 && rmag < wr1) {
                    const int j = window_bin(L.sed, nb, wlo, rmag, q);
                    double mu = 0;
                    if (MU || POLES) mu = mode_mu(g, rr, rmag);
                    const double *c = L.t1 + j * s1;
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
                        const int m = mu_bin(L.smu, nmu, mu, q.minv);
                        if (m >= 0) f += L.t2[j * nmu + m];
                    }
                    f *= P.volume;
                } else if (!(first && !(rmag >= rlo && rmag < rhi))) {
                    continue;                       // another pass holds the bin of this cell (pass_writes_zero, inline)
                }
                put(i0, i1, f);
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
    return launch_tiles(
        elsize, p, ntiles, lds, stream,
        [](auto c, auto m, auto pl) { return corr_kernel<typename decltype(c)::type, m, pl>; }, P, g, (const char *)x,
        redges, muedges, acc);
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
    return launch_tiles(
        elsize, p, ntiles, lds, stream,
        [](auto c, auto m, auto pl) { return corr_vjp_kernel<typename decltype(c)::type, m, pl>; }, P, g, (char *)gr,
        redges, muedges, coef);
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
