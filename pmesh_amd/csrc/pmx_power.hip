// pmx_power.hip — binned power spectrum of a complex field: P(k), P(k, mu) and multipoles in one read of the field.
//
// Replaces the reference's slab loop of numpy.digitize + bincount (TransferFunction.PowerSpectrum,
// pmesh/transfer.py:133-181), with the semantics of include/pmesh_amd.h (pmx_power_project).  HBM-bound: one read of
// a (and b) per mode, wavenumbers recomputed from the index, no mesh-sized temporaries, no per-mode global atomics.
//
// A workgroup takes a tile of PT0 x PT1 x PT2 modes along the memory-order axes (PT2 along the fastest one, one
// wave wide, so that a wave reads contiguous memory).  |k| is monotone in every |k_d|, so the tile's |k| range, and
// with it the range of k bins it can touch, follows from the extreme |k_d| of its index box in the same rounded
// arithmetic as the modes themselves: the workgroup keeps only that window of bins in LDS (at most `window` bins per
// pass; a tile that spans more bins — very fine edges — is read once per window).  Within a wave, a thread walks its
// rows in sequence and sums runs of modes that fall in the same bin (cell) in registers, so the LDS atomics happen
// once per run instead of once per mode; the window is added to the global accumulator once per tile, bins that
// received nothing skipped.
//
// The tile walk — LDS layout, tile prologue, row split, window loop, run sums, Hermitian weight, sinc division and the
// <T, MU, POLES> launch — is the skeleton of pmx_power_dev.h, shared with power_vjp_kernel, corr_kernel and
// corr_vjp_kernel; this file keeps what a mode contributes and to which sums.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_power_dev.h"

namespace pmx {

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) power_kernel(PParams P, PGeom g, const char *__restrict__ a,
                                                       const char *__restrict__ b, const double *__restrict__ kedges,
                                                       const double *__restrict__ muedges, double *__restrict__ acc)
{
    extern __shared__ double sm[];
    const PLds L = lds_layout<MU>(sm, P);           // t1: window * s1 sums, t2: window * nmu * 5
    const PTile t = tile_begin<false, MU>(P, g, L, kedges, muedges);
    if (t.bhi < t.blo) return;

    const int lane = threadIdx.x & 63;
    const PGuess q = bin_guess<MU>(P, L, kedges);
    const PRows w = wave_rows(t);
    const double k2ax = L.kax[2 * 64 + lane], s2ax = L.sax[2 * 64 + lane];
    const int64_t offa2 = lane_off(t, g.sa), offb2 = lane_off(t, g.sb);
    const int s1 = P.s1, nmu = P.nmu;
    int64_t ilast_fixed = -1;
    if (g.alast == 2) ilast_fixed = g.start[2] + t.o[2] + lane;

    for (int wlo = t.blo; wlo <= t.bhi; wlo += P.window) {
        const int nb = window_edges(P, t, wlo, L.sed, kedges);
        window_zero(L.t1, nb * s1);
        if (MU) window_zero(L.t2, nb * nmu * 5);
        __syncthreads();
        const double wk0 = L.sed[0], wk1 = L.sed[nb];

        Run<POLES ? 4 + 2 * PMX_POWER_MAX_POLES : 4> r1d;
        Run<5> rp, rm;
        r1d.reset(-1);
        rp.reset(-1);
        rm.reset(-1);
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
                if (!(kmag >= wk0 && kmag < wk1)) continue;
                const int j = window_bin(L.sed, nb, wlo, kmag, q);
                double vr, vi;
                if (P.cross) {
                    vr = ar[u] * br[u] + ai[u] * bi[u];
                    vi = ai[u] * br[u] - ar[u] * bi[u];
                } else {
                    vr = ar[u] * ar[u] + ai[u] * ai[u];
                    vi = 0;
                }
                vr *= P.volume;
                vi *= P.volume;
                if (P.deconv_pow) sinc_divide(g, L.sax[i0], L.sax[64 + i1], s2ax, vr, vi);
                const bool h = mode_hermitian(P, g, t, ilast_fixed, i0, i1);
                double mu = 0;
                if (MU || POLES) mu = mode_mu(g, kk, kmag);

                // 1-d table: the mode and (h) its conjugate at -mu
                r1d.select(j, L.t1, s1);
                r1d.s[0] += h ? 2.0 : 1.0;
                r1d.s[1] += h ? 2.0 * kmag : kmag;
                r1d.s[2] += h ? 2.0 * vr : vr;
                r1d.s[3] += h ? 0.0 : vi;
                if (POLES) {
                    double lp[PMX_POWER_MAX_POLES];
                    legendre_poles(P, mu, lp);
#pragma unroll
                    for (int p = 0; p < PMX_POWER_MAX_POLES; p++) {
                        if (p >= P.npoles) break;
                        const bool odd = P.poles[p] & 1;
                        // v L(mu) + conj(v) L(-mu), L(-mu) = (-1)^ell L(mu)
                        r1d.s[4 + 2 * p] += h ? (odd ? 0.0 : 2.0 * vr * lp[p]) : vr * lp[p];
                        r1d.s[5 + 2 * p] += h ? (odd ? 2.0 * vi * lp[p] : 0.0) : vi * lp[p];
                    }
                }
                if (MU) {
                    const int mp = mu_bin(L.smu, nmu, mu, q.minv);
                    const int cp = mp < 0 ? -1 : j * nmu + mp;
                    if (cp >= 0) {
                        rp.select(cp, L.t2, 5);
                        rp.s[0] += 1.0;
                        rp.s[1] += kmag;
                        rp.s[2] += mu;
                        rp.s[3] += vr;
                        rp.s[4] += vi;
                    }
                    if (h) {
                        const int mm = mu_bin(L.smu, nmu, -mu, q.minv);
                        const int cm = mm < 0 ? -1 : j * nmu + mm;
                        if (cm >= 0) {
                            rm.select(cm, L.t2, 5);
                            rm.s[0] += 1.0;
                            rm.s[1] += kmag;
                            rm.s[2] += -mu;
                            rm.s[3] += vr;
                            rm.s[4] += -vi;
                        }
                    }
                }
            }
        }
        r1d.flush(L.t1, s1, s1);
        if (MU) {
            rp.flush(L.t2, 5, 5);
            rm.flush(L.t2, 5, 5);
        }
        __syncthreads();
        window_add(acc + (int64_t)wlo * s1, L.t1, nb * s1, s1);
        if (MU) window_add(acc + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 5, L.t2, nb * nmu * 5, 5);
        __syncthreads();
    }
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_power_project(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a,
                                 const int64_t *a_strides, const void *b, const int64_t *b_strides,
                                 const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                 const double *boxsize, const double *kedges, const double *muedges, double *acc,
                                 void *stream)
{
    PMX_REQUIRE(acc, PMX_EINVAL, "bad arguments");
    PParams P;
    PGeom g;
    int64_t ntiles;
    size_t lds = 0;
    const int rc = power_setup(p, ndim, elsize, a, a_strides, b, b_strides, shape, start, nmesh, boxsize, kedges,
                               muedges, 4 + 2 * (p ? p->npoles : 0), 5, P, g, &ntiles, &lds);
    if (rc != PMX_OK || ntiles == 0) return rc;
    return launch_tiles(
        elsize, p, ntiles, lds, stream,
        [](auto c, auto m, auto pl) { return power_kernel<typename decltype(c)::type, m, pl>; }, P, g, (const char *)a,
        (const char *)b, kedges, muedges, acc);
}
