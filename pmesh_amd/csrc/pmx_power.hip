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

namespace pmx {

constexpr int PT0 = 16, PT1 = 16, PT2 = 64;   // tile extents along the memory-order axes (slowest .. fastest)
constexpr int PBLOCK = 256;
constexpr int PBATCH = 4;                     // rows whose loads are issued together
constexpr int PLDS_BUDGET = 5120;             // doubles of LDS per workgroup (40 KB: four workgroups per CU)
constexpr int PAXIS = 3 * 64;                 // per-axis tables of the tile: k_d and sinc(w_d/2)^p

struct PGeom {
    int64_t shape[3], sa[3], sb[3];           // memory order: [0] slowest .. [2] fastest
    int64_t start[3], nmesh[3];               // memory order
    double dw[3], nl_n[3], boxsize[3];        // 2 pi / N, N (as double), L per memory-order axis
    double los[3];                            // logical order
    int32_t ax[3];                            // logical axis of memory-order axis a
    int32_t on[3];                            // memory-order axis a is a mesh axis (not padding)
    int32_t alast;                            // memory-order position of the logical last axis
    int64_t nlast;                            // N of the logical last axis
    int32_t nt[3];                            // tiles along each memory-order axis
};

struct PParams {
    int32_t nk, nmu, npoles, window, hermitian, deconv_pow, cross, s1;
    int32_t poles[PMX_POWER_MAX_POLES];
    double volume;
};

// j in [0, n) with e[j] <= x < e[j + 1], for e[0] <= x < e[n]; the guess g is tried first (exact for uniform edges
// but for rounding at an edge, where the search takes over)
__device__ __forceinline__ int find_bin(const double *e, int n, double x, int g)
{
    g = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
    if (e[g] <= x && x < e[g + 1]) return g;
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        int m = (lo + hi) >> 1;
        if (e[m] <= x) lo = m;
        else hi = m;
    }
    return lo;
}

__device__ __forceinline__ int guess(double x, double e0, double inv)
{
    double t = (x - e0) * inv;
    return t < 0 ? 0 : (t > 1e9 ? 1000000000 : (int)t);
}

// the mu bin of mu (-1: outside muedges); the last bin is closed on the right
__device__ __forceinline__ int mu_bin(const double *e, int n, double mu, double inv)
{
    if (!(mu >= e[0] && mu <= e[n])) return -1;
    if (mu == e[n]) return n - 1;
    return find_bin(e, n, mu, guess(mu, e[0], inv));
}

// the number of the n values e[0] <= ... <= e[n-1] that are <= x, found by one wave: 64 probes per step
__device__ __forceinline__ int wave_upper(const double *e, int n, double x, int lane)
{
    int lo = 0, hi = n;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int step = (hi - lo + 63) / 64;
        const int pos = lo + lane * step;
        const bool le = pos < hi && e[pos] <= x;
        const int c = __popcll(__ballot(le));
        if (c == 0) break;                         // e[lo] > x
        const int nlo = lo + (c - 1) * step + 1;
        hi = min(hi, lo + c * step);
        lo = nlo;
    }
    return lo;
}

__device__ __forceinline__ double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename T> struct Cplx;
template <> struct Cplx<double> {
    static __device__ __forceinline__ void load(const char *p, double &re, double &im)
    {
        double2 v = *(const double2 *)p;
        re = v.x;
        im = v.y;
    }
};
template <> struct Cplx<float> {
    static __device__ __forceinline__ void load(const char *p, double &re, double &im)
    {
        float2 v = *(const float2 *)p;
        re = v.x;
        im = v.y;
    }
};

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
        const int ax = wv;
        double k = 0, sp = 1;
        if (lane < ext[ax] && g.on[ax]) {
            const int64_t gi = g.start[ax] + o[ax] + lane;
            double s = (double)gi;
            if (gi >= g.nmesh[ax] / 2) s -= (double)g.nmesh[ax];
            const double w = s * g.dw[ax];                  // 2 pi / N first, as pm.py:_block_coords does
            k = (w * g.nl_n[ax]) / g.boxsize[ax];
            if (P.deconv_pow) {
                const double x = 0.5 * w;
                double sn;
                if (x < 1e-5 && x > -1e-5) { double x2 = x * x; sn = 1.0 - x2 / 6. + x2 * x2 / 120.; }
                else sn = sin(x) / x;
                sp = sn;
                for (int e = 1; e < P.deconv_pow; e++) sp *= sn;
            }
        }
        kax[ax * 64 + lane] = k;
        sax[ax * 64 + lane] = sp;
        const bool in = lane < ext[ax];
        const double mn = wave_min(in ? fabs(k) : INFINITY), mx = wave_max(in ? fabs(k) : 0.0);
        if (lane == 0) { s_ext[ax][0] = mn; s_ext[ax][1] = mx; }
    } else if (MU) {
        for (int i = lane; i <= P.nmu; i += 64) smu[i] = muedges[i];
    }
    __syncthreads();
    if (wv < 2) {
        // |k| of the nearest (wave 0) / farthest (wave 1) corner, summed in logical axis order (monotone in every
        // |k_d|), and the number of edges at or below it
        double m[3] = {0, 0, 0};
        for (int ax = 0; ax < 3; ax++) m[g.ax[ax]] = s_ext[ax][wv];
        const int u = wave_upper(kedges, P.nk + 1, sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]), lane);
        if (lane == 0) s_range[wv] = wv == 0 ? (u > 0 ? u - 1 : 0) : (u - 1 < P.nk - 1 ? u - 1 : P.nk - 1);
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
                    Cplx<T>::load(a + (o[0] + i0) * g.sa[0] + (o[1] + i1) * g.sa[1] + offa2, ar[u], ai[u]);
                    if (P.cross)
                        Cplx<T>::load(b + (o[0] + i0) * g.sb[0] + (o[1] + i1) * g.sb[1] + offb2, br[u], bi[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < PBATCH; u++) {
                const int r = rb + u;
                if (!(r < r1 && lane_on)) continue;
                const int i0 = r / ext[1], i1 = r - i0 * ext[1];
                const double km[3] = {kax[i0], kax[64 + i1], k2ax};
                double kk[3];
#pragma unroll
                for (int d = 0; d < 3; d++) kk[d] = g.ax[0] == d ? km[0] : (g.ax[1] == d ? km[1] : km[2]);
                const double kmag = sqrt((kk[0] * kk[0] + kk[1] * kk[1]) + kk[2] * kk[2]);
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
                if (MU || POLES)
                    if (kmag > 0) mu = ((kk[0] * g.los[0] + kk[1] * g.los[1]) + kk[2] * g.los[2]) / kmag;

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
                    // Legendre polynomials by their recurrence (n + 1) L_{n+1} = (2n + 1) mu L_n - n L_{n-1}
                    double lm1 = 1.0, l0 = mu;
                    double lp[PMX_POWER_MAX_POLES];
#pragma unroll
                    for (int p = 0; p < PMX_POWER_MAX_POLES; p++) lp[p] = P.poles[p] == 0 ? 1.0 : mu;
#pragma unroll
                    for (int n = 1; n < PMX_POWER_MAX_ELL; n++) {
                        const double ln = ((2 * n + 1) * mu * l0 - n * lm1) / (n + 1);
                        lm1 = l0;
                        l0 = ln;
#pragma unroll
                        for (int p = 0; p < PMX_POWER_MAX_POLES; p++)
                            if (P.poles[p] == n + 1) lp[p] = ln;
                    }
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

template <typename T, bool MU, bool POLES>
static void launch(dim3 grid, size_t lds, hipStream_t st, const PParams &P, const PGeom &g, const void *a,
                   const void *b, const double *ke, const double *me, double *acc)
{
    power_kernel<T, MU, POLES><<<grid, PBLOCK, lds, st>>>(P, g, (const char *)a, (const char *)b, ke, me, acc);
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_power_project(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a,
                                 const int64_t *a_strides, const void *b, const int64_t *b_strides,
                                 const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                 const double *boxsize, const double *kedges, const double *muedges, double *acc,
                                 void *stream)
{
    PMX_REQUIRE(p && ndim >= 1 && ndim <= 3 && a && a_strides && shape && start && nmesh && boxsize && kedges && acc,
                PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(p->nk >= 1, PMX_EINVAL, "nk must be >= 1");
    PMX_REQUIRE(p->nk <= PMX_POWER_MAX_KBINS, PMX_EUNSUPPORTED, "nk above PMX_POWER_MAX_KBINS");
    PMX_REQUIRE(p->nmu >= 0 && p->npoles >= 0, PMX_EINVAL, "nmu, npoles must be >= 0");
    PMX_REQUIRE(p->nmu <= PMX_POWER_MAX_MUBINS, PMX_EUNSUPPORTED, "nmu above PMX_POWER_MAX_MUBINS");
    PMX_REQUIRE(p->npoles <= PMX_POWER_MAX_POLES, PMX_EUNSUPPORTED, "npoles above PMX_POWER_MAX_POLES");
    PMX_REQUIRE(p->nmu == 0 || muedges, PMX_EINVAL, "muedges needed for nmu > 0");
    PMX_REQUIRE(p->deconv_pow >= 0, PMX_EINVAL, "deconv_pow must be >= 0");
    PMX_REQUIRE(!b || b_strides, PMX_EINVAL, "b_strides needed with b");
    for (int i = 0; i < p->npoles; i++)
        PMX_REQUIRE(p->poles[i] >= 0 && p->poles[i] <= PMX_POWER_MAX_ELL, PMX_EUNSUPPORTED, "ell above PMX_POWER_MAX_ELL");

    PParams P;
    P.nk = p->nk;
    P.nmu = p->nmu;
    P.npoles = p->npoles;
    for (int i = 0; i < PMX_POWER_MAX_POLES; i++) P.poles[i] = i < p->npoles ? p->poles[i] : -1;
    P.hermitian = p->hermitian ? 1 : 0;
    P.deconv_pow = p->deconv_pow;
    P.cross = b ? 1 : 0;
    P.volume = p->volume;
    P.s1 = 4 + 2 * p->npoles;
    const int fixed = 2 * PAXIS + (p->nmu ? p->nmu + 1 : 0) + 1;
    P.window = (PLDS_BUDGET - fixed) / (P.s1 + 1 + 5 * p->nmu);
    PMX_REQUIRE(P.window >= 1, PMX_EUNSUPPORTED, "bin table does not fit");

    // memory order: axes of extent 1 slowest, then by decreasing stride of a
    int64_t sh[3], sa[3], sb[3], st[3], nm[3];
    double bx[3];
    for (int d = 0; d < 3; d++) {
        bool on = d < ndim;
        sh[d] = on ? shape[d] : 1;
        sa[d] = on ? a_strides[d] : 0;
        sb[d] = on && b ? b_strides[d] : 0;
        st[d] = on ? start[d] : 0;
        nm[d] = on ? nmesh[d] : 1;
        bx[d] = on ? boxsize[d] : 1.0;
        PMX_REQUIRE(sh[d] >= 0 && nm[d] >= 1, PMX_EINVAL, "bad shape");
    }
    int ax[3] = {0, 1, 2};
    auto before = [&](int x, int y) {   // x goes before (slower than) y
        bool ux = sh[x] == 1, uy = sh[y] == 1;
        if (ux != uy) return ux;
        return llabs(sa[x]) > llabs(sa[y]);
    };
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (before(ax[j], ax[i])) { int t = ax[i]; ax[i] = ax[j]; ax[j] = t; }
    PGeom g;
    for (int m = 0; m < 3; m++) {
        const int d = ax[m];
        g.ax[m] = d;
        g.on[m] = d < ndim;
        g.shape[m] = sh[d];
        g.sa[m] = sa[d];
        g.sb[m] = sb[d];
        g.start[m] = st[d];
        g.nmesh[m] = nm[d];
        g.dw[m] = 2 * M_PI / nm[d];
        g.nl_n[m] = (double)nm[d];
        g.boxsize[m] = bx[d];
        g.los[m] = p->los[m];
        if (d == ndim - 1) g.alast = m;
    }
    g.nlast = nmesh[ndim - 1];
    g.nt[0] = (int)((g.shape[0] + PT0 - 1) / PT0);
    g.nt[1] = (int)((g.shape[1] + PT1 - 1) / PT1);
    g.nt[2] = (int)((g.shape[2] + PT2 - 1) / PT2);
    const int64_t ntiles = (int64_t)g.nt[0] * g.nt[1] * g.nt[2];
    if (ntiles == 0 || g.shape[0] * g.shape[1] * g.shape[2] == 0) return PMX_OK;
    PMX_REQUIRE(ntiles < (1ll << 31), PMX_EUNSUPPORTED, "more than 2^31 tiles");

    const size_t lds = sizeof(double) * (size_t)(fixed + P.window * (P.s1 + 5 * p->nmu) + P.window);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ntiles);
    const bool mu = p->nmu > 0, poles = p->npoles > 0;
    if (elsize == 8) {
        if (mu && poles) launch<double, true, true>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else if (mu) launch<double, true, false>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else if (poles) launch<double, false, true>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else launch<double, false, false>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
    } else {
        if (mu && poles) launch<float, true, true>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else if (mu) launch<float, true, false>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else if (poles) launch<float, false, true>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
        else launch<float, false, false>(grid, lds, s, P, g, a, b, kedges, muedges, acc);
    }
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
