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
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_power_dev.h"

namespace pmx {

// the running sums of one thread for one key (a k bin, or a (k, mu) cell)
template <int N> struct Run {
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

template <typename T, bool MU, bool POLES>
__global__ void __launch_bounds__(PBLOCK) power_kernel(PParams P, PGeom g, const char *__restrict__ a,
                                                       const char *__restrict__ b, const double *__restrict__ kedges,
                                                       const double *__restrict__ muedges, double *__restrict__ acc)
{
    extern __shared__ double sm[];
    double *kax = sm;                               // [3][64]  k_d along each memory-order axis of the tile
    double *sax = sm + PAXIS;                       // [3][64]  sinc(w_d/2)^deconv_pow
    double *smu = sm + 2 * PAXIS;                   // nmu + 1
    double *sed = smu + (MU ? P.nmu + 1 : 0);       // window + 1 k edges
    double *t1 = sed + P.window + 1;                // window * s1
    double *t2 = t1 + P.window * P.s1;              // window * nmu * 5
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

    // per-axis tables of the tile and the extreme |k_d| over its index box (waves 0, 1, 2: one axis each)
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
    if (bhi < blo) return;

    const double ke0 = kedges[0], kinv = P.nk / (kedges[P.nk] - kedges[0]);
    const double minv = MU ? P.nmu / (smu[P.nmu] - smu[0]) : 0;
    const int nrows = ext[0] * ext[1];
    const int rper = (nrows + 3) / 4;
    const int r0 = wv * rper, r1 = min(nrows, r0 + rper);
    const bool lane_on = lane < ext[2];
    const double k2ax = kax[2 * 64 + lane], s2ax = sax[2 * 64 + lane];
    const int64_t offa2 = (o[2] + lane) * g.sa[2], offb2 = (o[2] + lane) * g.sb[2];
    const int s1 = P.s1, nmu = P.nmu;
    int64_t ilast_fixed = -1;
    if (g.alast == 2) ilast_fixed = g.start[2] + o[2] + lane;

    for (int wlo = blo; wlo <= bhi; wlo += P.window) {
        const int nb = min(P.window, bhi - wlo + 1);
        for (int i = tid; i < nb * s1; i += PBLOCK) t1[i] = 0;
        if (MU)
            for (int i = tid; i < nb * nmu * 5; i += PBLOCK) t2[i] = 0;
        for (int i = tid; i <= nb; i += PBLOCK) sed[i] = kedges[wlo + i];
        __syncthreads();
        const double wk0 = sed[0], wk1 = sed[nb];

        Run<POLES ? 4 + 2 * PMX_POWER_MAX_POLES : 4> r1d;
        Run<5> rp, rm;
        r1d.reset(-1);
        rp.reset(-1);
        rm.reset(-1);
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
                if (!(kmag >= wk0 && kmag < wk1)) continue;
                const int j = find_bin(sed, nb, kmag, guess(kmag, ke0, kinv) - wlo);
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
                if (P.deconv_pow) {
                    const double sm3[3] = {sax[i0], sax[64 + i1], s2ax};
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const double sp = g.ax[0] == d ? sm3[0] : (g.ax[1] == d ? sm3[1] : sm3[2]);
                        vr /= sp;
                        vi /= sp;
                    }
                }
                bool h = false;
                if (P.hermitian) {
                    const int64_t il = g.alast == 2 ? ilast_fixed
                                                    : g.start[g.alast] + o[g.alast] + (g.alast == 0 ? i0 : i1);
                    h = il != 0 && il != g.nlast / 2;
                }
                double mu = 0;
                if (MU || POLES) mu = mode_mu(g, kk, kmag);

                // 1-d table: the mode and (h) its conjugate at -mu
                if (j != r1d.key) {
                    r1d.flush(t1, s1, s1);
                    r1d.reset(j);
                }
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
                    const int mp = mu_bin(smu, nmu, mu, minv);
                    const int cp = mp < 0 ? -1 : j * nmu + mp;
                    if (cp >= 0) {
                        if (cp != rp.key) { rp.flush(t2, 5, 5); rp.reset(cp); }
                        rp.s[0] += 1.0;
                        rp.s[1] += kmag;
                        rp.s[2] += mu;
                        rp.s[3] += vr;
                        rp.s[4] += vi;
                    }
                    if (h) {
                        const int mm = mu_bin(smu, nmu, -mu, minv);
                        const int cm = mm < 0 ? -1 : j * nmu + mm;
                        if (cm >= 0) {
                            if (cm != rm.key) { rm.flush(t2, 5, 5); rm.reset(cm); }
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
        r1d.flush(t1, s1, s1);
        if (MU) {
            rp.flush(t2, 5, 5);
            rm.flush(t2, 5, 5);
        }
        __syncthreads();
        // the window into the global sums: contiguous runs of doubles, bins that received nothing skipped
        double *g1 = acc + (int64_t)wlo * s1;
        for (int i = tid; i < nb * s1; i += PBLOCK)
            if (t1[(i / s1) * s1] != 0) unsafeAtomicAdd(g1 + i, t1[i]);
        if (MU) {
            double *g2 = acc + (int64_t)P.nk * s1 + (int64_t)wlo * nmu * 5;
            for (int i = tid; i < nb * nmu * 5; i += PBLOCK)
                if (t2[(i / 5) * 5] != 0) unsafeAtomicAdd(g2 + i, t2[i]);
        }
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
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ntiles);
    const bool mu = p->nmu > 0, poles = p->npoles > 0;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mu, [&](auto m) {
            with_bool(poles, [&](auto pl) {
                power_kernel<T, m, pl><<<grid, PBLOCK, lds, s>>>(P, g, (const char *)a, (const char *)b, kedges, muedges, acc);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
