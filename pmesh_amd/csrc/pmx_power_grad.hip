// pmx_power_grad.hip — the adjoint of the binned power spectrum (include/pmesh_amd.h: pmx_power_vjp).
//
// A caller of the reference differentiates its spectrum through torch on materialised |k| and mu (bucketize +
// index_add_ and their backward); here one kernel reads a (and b) once and writes grad_a (and grad_b) once, in the
// memory order, tile shape and windows of power_kernel (pmx_power.hip), with the wavenumbers, bins and Legendre
// polynomials of pmx_power_dev.h, so that every mode lands in the bin the forward put it in.  Where the forward adds a
// mode's sums into the LDS window of its k bins, this kernel gathers the coefficients of the mode's bin (and (k, mu)
// cells) from an LDS window of the coefficient table the host built from the cotangents and the counts: no atomics,
// no run registers.  A tile that spans more bins than a window holds takes one pass per window, and each of its modes
// is written by exactly one pass: the pass whose window holds its bin, or the first one (zero) when it has no bin.
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
    double *kax = sm;                               // [3][64]  k_d along each memory-order axis of the tile
    double *sax = sm + PAXIS;                       // [3][64]  sinc(w_d/2)^deconv_pow
    double *smu = sm + 2 * PAXIS;                   // nmu + 1
    double *sed = smu + (MU ? P.nmu + 1 : 0);       // window + 1 k edges
    double *t1 = sed + P.window + 1;                // window * s1 coefficients of the k bins
    double *t2 = t1 + P.window * P.s1;              // window * nmu * 2 coefficients of the (k, mu) cells
    __shared__ double s_ext[3][2];
    __shared__ int s_range[2];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t tile = blockIdx.x;
    const int c2 = (int)(tile % g.nt[2]);
    tile /= g.nt[2];
    const int c1 = (int)(tile % g.nt[1]), c0 = (int)(tile / g.nt[1]);
    const int64_t o[3] = {(int64_t)c0 * PT0, (int64_t)c1 * PT1, (int64_t)c2 * PT2};
    const int ext[3] = {(int)min((int64_t)PT0, g.shape[0] - o[0]), (int)min((int64_t)PT1, g.shape[1] - o[1]),
                        (int)min((int64_t)PT2, g.shape[2] - o[2])};

    if (wv < 3) {
        tile_axis(P, g, wv, lane, ext[wv], o[wv], kax, sax, s_ext[wv]);
    } else if (MU) {
        for (int i = lane; i <= P.nmu; i += 64) smu[i] = muedges[i];
    }
    __syncthreads();
    if (wv < 2) {
        const int j = tile_bin_range(P, g, wv, lane, s_ext, kedges);
        if (lane == 0) s_range[wv] = j;
    }
    __syncthreads();
    const int blo = s_range[0], bhi = s_range[1];

    const int nrows = ext[0] * ext[1];
    const int rper = (nrows + 3) / 4;
    const int r0 = wv * rper, r1 = min(nrows, r0 + rper);
    const bool lane_on = lane < ext[2];
    const int64_t offa2 = (o[2] + lane) * g.sa[2], offb2 = (o[2] + lane) * g.sb[2];
    const int64_t offga2 = (o[2] + lane) * out.sga[2], offgb2 = (o[2] + lane) * out.sgb[2];

    if (bhi < blo) {
        // no mode of the tile has a k bin: zeros
        if (lane_on)
            for (int r = r0; r < r1; r++) {
                const int i0 = r / ext[1], i1 = r - i0 * ext[1];
                CLoad<T>::put(out.ga + (o[0] + i0) * out.sga[0] + (o[1] + i1) * out.sga[1] + offga2, 0.0, 0.0);
                if (P.cross)
                    CLoad<T>::put(out.gb + (o[0] + i0) * out.sgb[0] + (o[1] + i1) * out.sgb[1] + offgb2, 0.0, 0.0);
            }
        return;
    }

    const double ke0 = kedges[0], kinv = P.nk / (kedges[P.nk] - kedges[0]);
    const double klo = kedges[blo], khi = kedges[bhi + 1];     // the tile's passes cover [klo, khi)
    const double minv = MU ? P.nmu / (smu[P.nmu] - smu[0]) : 0;
    const double k2ax = kax[2 * 64 + lane], s2ax = sax[2 * 64 + lane];
    const int s1 = P.s1, nmu = P.nmu;
    int64_t ilast_fixed = -1;
    if (g.alast == 2) ilast_fixed = g.start[2] + o[2] + lane;

    for (int wlo = blo; wlo <= bhi; wlo += P.window) {
        const int nb = min(P.window, bhi - wlo + 1);
        const double *g1 = coef + (int64_t)wlo * s1;
        for (int i = tid; i < nb * s1; i += PBLOCK) t1[i] = g1[i];
        if (MU) {
            const double *g2 = coef + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 2;
            for (int i = tid; i < nb * nmu * 2; i += PBLOCK) t2[i] = g2[i];
        }
        for (int i = tid; i <= nb; i += PBLOCK) sed[i] = kedges[wlo + i];
        __syncthreads();
        const double wk0 = sed[0], wk1 = sed[nb];
        const bool first = wlo == blo;

        for (int rb = r0; rb < r1; rb += PBATCH) {
            double ar[PBATCH], ai[PBATCH], br[PBATCH], bi[PBATCH];
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                ar[u] = ai[u] = br[u] = bi[u] = 0;
                if (r < r1 && lane_on) {
                    const int i0 = r / ext[1], i1 = r - i0 * ext[1];
                    CLoad<T>::get(a + (o[0] + i0) * g.sa[0] + (o[1] + i1) * g.sa[1] + offa2, ar[u], ai[u]);
                    if (P.cross)
                        CLoad<T>::get(b + (o[0] + i0) * g.sb[0] + (o[1] + i1) * g.sb[1] + offb2, br[u], bi[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                if (!(r < r1 && lane_on)) continue;
                const int i0 = r / ext[1], i1 = r - i0 * ext[1];
                const double km[3] = {kax[i0], kax[64 + i1], k2ax};
                double kk[3];
                const double kmag = mode_k(g, km[0], km[1], km[2], kk);
                double gar = 0, gai = 0, gbr = 0, gbi = 0;
                if (kmag >= wk0 && kmag < wk1) {
                    const int j = find_bin(sed, nb, kmag, guess(kmag, ke0, kinv) - wlo);
                    bool h = false;
                    if (P.hermitian) {
                        const int64_t il = g.alast == 2 ? ilast_fixed
                                                        : g.start[g.alast] + o[g.alast] + (g.alast == 0 ? i0 : i1);
                        h = il != 0 && il != g.nlast / 2;
                    }
                    double mu = 0;
                    if (MU || POLES) mu = mode_mu(g, kk, kmag);
                    // F(mu) and F(-mu): the coefficients of the mode's bin, pole by pole and cell by cell
                    const double *c = t1 + j * s1;
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
                        const int mp = mu_bin(smu, nmu, mu, minv);
                        if (mp >= 0) {
                            fpr += t2[(j * nmu + mp) * 2];
                            fpi += t2[(j * nmu + mp) * 2 + 1];
                        }
                        if (h) {
                            const int mm = mu_bin(smu, nmu, -mu, minv);
                            if (mm >= 0) {
                                fmr += t2[(j * nmu + mm) * 2];
                                fmi += t2[(j * nmu + mm) * 2 + 1];
                            }
                        }
                    }
                    // q = (V / D) (conj(F(mu)) + h F(-mu)), over the weight of the mode
                    double qr = h ? fpr + fmr : fpr, qi = h ? fmi - fpi : -fpi;
                    qr *= P.volume;
                    qi *= P.volume;
                    if (P.deconv_pow) {
                        const double sm3[3] = {sax[i0], sax[64 + i1], s2ax};
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            const double sp = g.ax[0] == d ? sm3[0] : (g.ax[1] == d ? sm3[1] : sm3[2]);
                            qr /= sp;
                            qi /= sp;
                        }
                    }
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
                } else if (!(first && !(kmag >= klo && kmag < khi))) {
                    continue;                       // another pass holds the bin of this mode
                }
                CLoad<T>::put(out.ga + (o[0] + i0) * out.sga[0] + (o[1] + i1) * out.sga[1] + offga2, gar, gai);
                if (P.cross)
                    CLoad<T>::put(out.gb + (o[0] + i0) * out.sgb[0] + (o[1] + i1) * out.sgb[1] + offgb2, gbr, gbi);
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
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ntiles);
    const bool mu = p->nmu > 0, poles = p->npoles > 0;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mu, [&](auto m) {
            with_bool(poles, [&](auto pl) {
                power_vjp_kernel<T, m, pl><<<grid, PBLOCK, lds, s>>>(P, g, o, (const char *)a, (const char *)b, kedges, muedges,
                                                                    coef);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
