// pmx_power_grad.hip — the adjoint of the binned power spectrum (include/pmesh_amd.h: pmx_power_vjp).
//
// A caller of the reference differentiates its spectrum through torch on materialised |k| and mu (bucketize +
// index_add_ and their backward); here one kernel reads a (and b) once and writes grad_a (and grad_b) once, in the
// memory order, tile shape and windows of power_kernel (pmx_power.hip) — both are written in the skeleton of
// pmx_power_dev.h: its tile prologue, row split, window loop, bins, Hermitian weight, sinc division and Legendre
// polynomials — so that every mode lands in the bin the forward put it in.  Where the forward adds a
// mode's sums into the LDS window of its k bins, this kernel gathers the coefficients of the mode's bin (and (k, mu)
// cells) from an LDS window of the coefficient table the host built from the cotangents and the counts: no atomics,
// no run registers.  A tile that spans more bins than a window holds takes one pass per window, and each of its modes
// is written by exactly one pass (pass_writes_zero and tile_zero of pmx_power_dev.h).
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_power_dev.h"

namespace pmx {

struct PGrad {
    char *ga, *gb;
    int64_t sga[3], sgb[3];                   // byte strides, memory order of a
};

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) power_vjp_kernel(PParams P, PGeom g, PGrad out, const char *__restrict__ a,
                                                           const char *__restrict__ b,
                                                           const double *__restrict__ kedges,
                                                           const double *__restrict__ muedges,
                                                           const double *__restrict__ coef)
{
    extern __shared__ double sm[];
    const PLds L = lds_layout<MU>(sm, P);           // t1: window * s1 coefficients, t2: window * nmu * 2
    const PTile t = tile_begin<false, MU>(P, g, L, kedges, muedges);

    const int lane = threadIdx.x & 63;
    const PRows w = wave_rows(t);
    const int64_t offa2 = lane_off(t, g.sa), offb2 = lane_off(t, g.sb);
    const int64_t offga2 = lane_off(t, out.sga), offgb2 = lane_off(t, out.sgb);
    auto put = [&](int i0, int i1, double gar, double gai, double gbr, double gbi) {
        CLoad<T>::put(row_ptr(out.ga, t, out.sga, i0, i1, offga2), gar, gai);
        if (P.cross) CLoad<T>::put(row_ptr(out.gb, t, out.sgb, i0, i1, offgb2), gbr, gbi);
    };
    if (t.bhi < t.blo) {
        tile_zero(t, w, [&](int i0, int i1) { put(i0, i1, 0.0, 0.0, 0.0, 0.0); });
        return;
    }

    const PGuess q = bin_guess<MU>(P, L, kedges);
    const double klo = kedges[t.blo], khi = kedges[t.bhi + 1];     // the tile's passes cover [klo, khi)
    const double k2ax = L.kax[2 * 64 + lane], s2ax = L.sax[2 * 64 + lane];
    const int s1 = P.s1, nmu = P.nmu;
    int64_t ilast_fixed = -1;
    if (g.alast == 2) ilast_fixed = g.start[2] + t.o[2] + lane;

    for (int wlo = t.blo; wlo <= t.bhi; wlo += P.window) {
        const int nb = window_edges(P, t, wlo, L.sed, kedges);
        window_load(L.t1, nb * s1, coef + (int64_t)wlo * s1);
        if (MU) window_load(L.t2, nb * nmu * 2, coef + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 2);
        __syncthreads();
        const double wk0 = L.sed[0], wk1 = L.sed[nb];
        const bool first = wlo == t.blo;

        for (int rb = w.r0; rb < w.r1; rb += PBATCH) {
            double ar[PBATCH], ai[PBATCH], br[PBATCH], bi[PBATCH];
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                ar[u] = ai[u] = br[u] = bi[u] = 0;
                if (r < w.r1 && w.lane_on) {
                    int i0, i1;
                    row_index(t, r, i0, i1);
                    CLoad<T>::get(row_ptr(a, t, g.sa, i0, i1, offa2), ar[u], ai[u]);
                    if (P.cross) CLoad<T>::get(row_ptr(b, t, g.sb, i0, i1, offb2), br[u], bi[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                if (!(r < w.r1 && w.lane_on)) continue;
                int i0, i1;
                row_index(t, r, i0, i1);
                double kk[3];
                const double kmag = mode_k(g, L.kax[i0], L.kax[64 + i1], k2ax, kk);
                double gar = 0, gai = 0, gbr = 0, gbi = 0;
                if (kmag >= wk0 && kmag < wk1) {
                    const int j = window_bin(L.sed, nb, wlo, kmag, q);
                    const bool h = mode_hermitian(P, g, t, ilast_fixed, i0, i1);
                    double mu = 0;
                    if (MU || POLES) mu = mode_mu(g, kk, kmag);
                    // F(mu) and F(-mu): the coefficients of the mode's bin, pole by pole and cell by cell
                    const double *c = L.t1 + j * s1;
                    double fpr = c[0], fpi = c[1], fmr = c[0], fmi = c[1];
                    if (POLES) {
                        double lp[PMX_POWER_MAX_POLES];
                        legendre_poles(P, mu, lp);
#pragma unroll
                        for (int p = 0; p < PMX_POWER_MAX_POLES; p++) {
                            if (p >= P.npoles) break;
                            const double cr = lp[p] * c[2 + 2 * p], ci = lp[p] * c[3 + 2 * p];
                            const bool odd = P.poles[p] & 1;        // L(-mu) = (-1)^ell L(mu)
                            fpr += cr;
                            fpi += ci;
                            fmr += odd ? -cr : cr;
                            fmi += odd ? -ci : ci;
                        }
                    }
                    if (MU) {
                        const int mp = mu_bin(L.smu, nmu, mu, q.minv);
                        if (mp >= 0) {
                            fpr += L.t2[(j * nmu + mp) * 2];
                            fpi += L.t2[(j * nmu + mp) * 2 + 1];
                        }
                        if (h) {
                            const int mm = mu_bin(L.smu, nmu, -mu, q.minv);
                            if (mm >= 0) {
                                fmr += L.t2[(j * nmu + mm) * 2];
                                fmi += L.t2[(j * nmu + mm) * 2 + 1];
                            }
                        }
                    }
                    // q = (V / D) (conj(F(mu)) + h F(-mu)), over the weight of the mode
                    double qr = h ? fpr + fmr : fpr, qi = h ? fmi - fpi : -fpi;
                    qr *= P.volume;
                    qi *= P.volume;
                    if (P.deconv_pow) sinc_divide(g, L.sax[i0], L.sax[64 + i1], s2ax, qr, qi);
                    if (h) {
                        qr *= 0.5;
                        qi *= 0.5;
                    }
                    if (P.cross) {
                        // grad_a = conj(q) b, grad_b = q a
                        gar = qr * br[u] + qi * bi[u];
                        gai = qr * bi[u] - qi * br[u];
                        gbr = qr * ar[u] - qi * ai[u];
                        gbi = qr * ai[u] + qi * ar[u];
                    } else {
                        gar = (2.0 * qr) * ar[u];
                        gai = (2.0 * qr) * ai[u];
                    }
                } else if (!pass_writes_zero(first, kmag, klo, khi)) {
                    continue;                       // another pass holds the bin of this mode
                }
                put(i0, i1, gar, gai, gbr, gbi);
            }
        }
        __syncthreads();
    }
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_power_vjp(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a, const int64_t *a_strides,
                             const void *b, const int64_t *b_strides, void *grad_a, const int64_t *grad_a_strides,
                             void *grad_b, const int64_t *grad_b_strides, const int64_t *shape, const int64_t *start,
                             const int64_t *nmesh, const double *boxsize, const double *kedges, const double *muedges,
                             const double *coef, void *stream)
{
    PMX_REQUIRE(coef && grad_a && grad_a_strides, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(!b == !grad_b && (!grad_b || grad_b_strides), PMX_EINVAL, "grad_b and its strides go with b");
    PMX_REQUIRE(grad_a != a && grad_a != b && (!grad_b || (grad_b != a && grad_b != b && grad_b != grad_a)), PMX_EINVAL,
                "the gradients must not alias the fields");
    PParams P;
    PGeom g;
    int64_t ntiles;
    size_t lds = 0;
    const int rc = power_setup(p, ndim, elsize, a, a_strides, b, b_strides, shape, start, nmesh, boxsize, kedges,
                               muedges, 2 + 2 * (p ? p->npoles : 0), 2, P, g, &ntiles, &lds);
    if (rc != PMX_OK || ntiles == 0) return rc;
    PGrad o;
    o.ga = (char *)grad_a;
    o.gb = (char *)grad_b;
    for (int m = 0; m < 3; m++) {
        const int d = g.ax[m];
        o.sga[m] = d < ndim ? grad_a_strides[d] : 0;
        o.sgb[m] = d < ndim && grad_b ? grad_b_strides[d] : 0;
    }
    return launch_tiles(
        elsize, p, ntiles, lds, stream,
        [](auto c, auto m, auto pl) { return power_vjp_kernel<typename decltype(c)::type, m, pl>; }, P, g, o,
        (const char *)a, (const char *)b, kedges, muedges, coef);
}
