// pmx_power_dev.h — the tile walk of the binned two-point statistics: what power_kernel (pmx_power.hip), its adjoint
// power_vjp_kernel (pmx_power_grad.hip) and corr_kernel / corr_vjp_kernel (pmx_corr.hip) share, so that every mode
// (cell) lands in the bin the forward put it in.  In reading order: the tile geometry and parameters; find_bin / guess /
// mu_bin;
// the per-axis tables of a tile on the k side (tile_axis) and the real side (tile_axis_real) with the extreme |k_d| of
// its index box; mode_k / mode_mu / the Legendre recurrence; then the skeleton every tile kernel is written in — the
// LDS layout next to the host formula that sizes it (PLds, lds_layout, lds_window, lds_doubles), the tile prologue
// (tile_begin), the row split (wave_rows, row_index, row_ptr), the window loop (window_edges, window_zero, window_load,
// window_bin, window_add), the running sums of the forwards (Run), the adjoints' rule for who writes an element
// (pass_writes_zero, tile_zero), the Hermitian weight and the sinc division of the k side (mode_hermitian,
// sinc_divide) — and the host side: power_setup, which orders the axes and sizes the window, and launch_tiles, the
// <T, MU, POLES> dispatch.  The wavenumber (k_divided), the sinc power, the complex loads and the axis-order rule come
// from pmx_block_dev.h.  The arithmetic is the forward's, statement for statement (-ffp-contract=off keeps its
// roundings).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

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

// s1: doubles per k bin of the table a tile keeps a window of in LDS (the forward's sums, the adjoint's coefficients)
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

// one wave per axis: lane's k_d and sinc(w_d/2)^deconv_pow along memory-order axis `ax` of the tile (extent ext, from
// index o there) into kax / sax, and the extreme |k_d| over the tile's index box into ext2 (min, max)
__device__ __forceinline__ void tile_axis(const PParams &P, const PGeom &g, int ax, int lane, int ext, int64_t o,
                                          double *kax, double *sax, double *ext2)
{
    double k = 0, sp = 1;
    if (lane < ext && g.on[ax]) {
        const double w = mode_w(g.start[ax] + o + lane, g.nmesh[ax], g.dw[ax]);
        k = k_divided(w, g.nl_n[ax], g.boxsize[ax]);    // as pm.py:_block_coords does
        if (P.deconv_pow) sp = sinc_pow(w, P.deconv_pow);
    }
    kax[ax * 64 + lane] = k;
    sax[ax * 64 + lane] = sp;
    const bool in = lane < ext;
    const double mn = wave_min(in ? fabs(k) : INFINITY), mx = wave_max(in ? fabs(k) : 0.0);
    if (lane == 0) { ext2[0] = mn; ext2[1] = mx; }
}

// wave 0 / wave 1: the first / last k bin the tile can touch, from |k| of the nearest / farthest corner of its index
// box (s_ext[axis][0 / 1]), summed in logical axis order (monotone in every |k_d|), and the number of edges at or
// below it
__device__ __forceinline__ int tile_bin_range(const PParams &P, const PGeom &g, int wv, int lane,
                                              const double (*s_ext)[2], const double *kedges)
{
    double m[3] = {0, 0, 0};
    for (int ax = 0; ax < 3; ax++) m[g.ax[ax]] = s_ext[ax][wv];
    const int u = wave_upper(kedges, P.nk + 1, sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]), lane);
    return wv == 0 ? (u > 0 ? u - 1 : 0) : (u - 1 < P.nk - 1 ? u - 1 : P.nk - 1);
}

// the wavevector of a mode in logical axis order from its per-axis values in memory order, and |k|
__device__ __forceinline__ double mode_k(const PGeom &g, double km0, double km1, double km2, double *kk)
{
#pragma unroll
    for (int d = 0; d < 3; d++) kk[d] = g.ax[0] == d ? km0 : (g.ax[1] == d ? km1 : km2);
    return sqrt((kk[0] * kk[0] + kk[1] * kk[1]) + kk[2] * kk[2]);
}

__device__ __forceinline__ double mode_mu(const PGeom &g, const double *kk, double kmag)
{
    double mu = 0;
    if (kmag > 0) mu = ((kk[0] * g.los[0] + kk[1] * g.los[1]) + kk[2] * g.los[2]) / kmag;
    return mu;
}

// lp[p] = L_ell_p(mu): Legendre polynomials by their recurrence (n + 1) L_{n+1} = (2n + 1) mu L_n - n L_{n-1}
__device__ __forceinline__ void legendre_poles(const PParams &P, double mu, double *lp)
{
    double lm1 = 1.0, l0 = mu;
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
}

// ---- the real side (pmx_corr.hip): a tile of a real mesh binned by the separation of its cells --------------------

// one real element of f4 / f8 storage, as a double
template <typename T> __device__ __forceinline__ double real_get(const char *p) { return (double)*(const T *)p; }
template <typename T> __device__ __forceinline__ void real_put(char *p, double v) { *(T *)p = (T)v; }

// r_d = (s * L) / N of global index gi (counted negative at and beyond N / 2): the Python expression
// `signed * BoxSize[d] / Nmesh[d]` of pm.py:_block_coords, what RealField.x holds on an f8 mesh
__device__ __forceinline__ double cell_r(int64_t gi, int64_t n, double nd, double L)
{
    double s = (double)gi;
    if (gi >= n / 2) s -= nd;
    return (s * L) / nd;
}

// tile_axis on the real side: lane's r_d along memory-order axis `ax` of the tile into rax, and the extreme |r_d| over
// the tile's index box into ext2 (min, max; a tile that straddles N / 2 holds both signs, the extremes are taken over
// its cells)
__device__ __forceinline__ void tile_axis_real(const PGeom &g, int ax, int lane, int ext, int64_t o, double *rax,
                                               double *ext2)
{
    double r = 0;
    if (lane < ext && g.on[ax]) r = cell_r(g.start[ax] + o + lane, g.nmesh[ax], g.nl_n[ax], g.boxsize[ax]);
    rax[ax * 64 + lane] = r;
    const bool in = lane < ext;
    const double mn = wave_min(in ? fabs(r) : INFINITY), mx = wave_max(in ? fabs(r) : 0.0);
    if (lane == 0) { ext2[0] = mn; ext2[1] = mx; }
}

// ---- the skeleton of a tile kernel ---------------------------------------------------------------------------------

// The dynamic LDS block of a workgroup, in doubles: two per-axis tables of the tile (the real side leaves the second
// one unused), the mu edges, the k edges of the window, and the window of the bin table (s1 doubles per k bin) and of
// the cell table (per_cell doubles per (k, mu) cell).  lds_layout carves what lds_window / lds_doubles size.
struct PLds {
    double *kax, *sax;                        // [3][64] each: k_d (r_d) and sinc(w_d/2)^deconv_pow along each axis
    double *smu, *sed;                        // nmu + 1 mu edges (with MU), window + 1 k edges
    double *t1, *t2;                          // window * s1, window * nmu * per_cell
};

constexpr int lds_fixed(int nmu) { return 2 * PAXIS + (nmu ? nmu + 1 : 0) + 1; }
constexpr int lds_window(int nmu, int s1, int per_cell)
{
    return (PLDS_BUDGET - lds_fixed(nmu)) / (s1 + 1 + per_cell * nmu);
}
constexpr size_t lds_doubles(int nmu, int s1, int per_cell, int window)
{
    return (size_t)(lds_fixed(nmu) + window * (s1 + per_cell * nmu) + window);
}

template <bool MU> __device__ __forceinline__ PLds lds_layout(double *sm, const PParams &P)
{
    PLds L;
    L.kax = sm;
    L.sax = sm + PAXIS;
    L.smu = sm + 2 * PAXIS;
    L.sed = L.smu + (MU ? P.nmu + 1 : 0);
    L.t1 = L.sed + P.window + 1;
    L.t2 = L.t1 + P.window * P.s1;
    return L;
}

// the tile of this workgroup: its origin and ragged extents along the memory-order axes, and the k bins blo .. bhi it
// can touch (none: bhi < blo)
struct PTile {
    int64_t o[3];
    int ext[3];
    int blo, bhi;
};

// What every tile kernel begins with: the tile of blockIdx.x, its per-axis tables (waves 0, 1, 2: one axis each; REAL:
// separations, else wavenumbers and sinc powers), the mu edges (wave 3) and its range of bins.
template <bool REAL, bool MU>
__device__ __forceinline__ PTile tile_begin(const PParams &P, const PGeom &g, const PLds &L, const double *edges,
                                            const double *muedges)
{
    __shared__ double s_ext[3][2];
    __shared__ int s_range[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    PTile t;
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
    // (selects, not t.ext[wv]: an index that is not a constant would put the tile into scratch memory)
    if (wv < 3) {
        const int e = wv == 0 ? t.ext[0] : (wv == 1 ? t.ext[1] : t.ext[2]);
        const int64_t o = wv == 0 ? t.o[0] : (wv == 1 ? t.o[1] : t.o[2]);
        if (REAL) tile_axis_real(g, wv, lane, e, o, L.kax, s_ext[wv]);
        else tile_axis(P, g, wv, lane, e, o, L.kax, L.sax, s_ext[wv]);
    } else if (MU) {
        for (int i = lane; i <= P.nmu; i += 64) L.smu[i] = muedges[i];
    }
    __syncthreads();
    if (wv < 2) {
        const int j = tile_bin_range(P, g, wv, lane, s_ext, edges);
        if (lane == 0) s_range[wv] = j;
    }
    __syncthreads();
    t.blo = s_range[0];
    t.bhi = s_range[1];
    return t;
}

// the rows r0 .. r1 - 1 of the tile this wave walks (row r = i0 * ext[1] + i1, a quarter of them per wave), and
// whether this lane holds an element of each
struct PRows {
    int r0, r1;
    bool lane_on;
};

__device__ __forceinline__ PRows wave_rows(const PTile &t)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nrows = t.ext[0] * t.ext[1], rper = (nrows + 3) / 4;
    PRows w;
    w.r0 = wv * rper;
    w.r1 = min(nrows, w.r0 + rper);
    w.lane_on = lane < t.ext[2];
    return w;
}

__device__ __forceinline__ void row_index(const PTile &t, int r, int &i0, int &i1)
{
    i0 = r / t.ext[1];
    i1 = r - i0 * t.ext[1];
}

// this lane's element of row (i0, i1) in a field at `base` of byte strides s (memory order); off2 = lane_off(t, s), the
// part that no row changes.  (The sum stays a chain from `base`, as the kernels wrote it: summed apart and added to the
// pointer at the end it cost power_vjp_kernel<MU, POLES> five registers and a wave per SIMD.)
__device__ __forceinline__ int64_t lane_off(const PTile &t, const int64_t *s)
{
    return (t.o[2] + (threadIdx.x & 63)) * s[2];
}
template <typename C>
__device__ __forceinline__ C *row_ptr(C *base, const PTile &t, const int64_t *s, int i0, int i1, int64_t off2)
{
    return base + (t.o[0] + i0) * s[0] + (t.o[1] + i1) * s[1] + off2;
}

// the guesses of the uniform edges: find_bin's first try among the k edges, mu_bin's among the mu edges
struct PGuess {
    double e0, inv, minv;
};

template <bool MU>
__device__ __forceinline__ PGuess bin_guess(const PParams &P, const PLds &L, const double *edges)
{
    PGuess q;
    q.e0 = edges[0];
    q.inv = P.nk / (edges[P.nk] - edges[0]);
    q.minv = MU ? P.nmu / (L.smu[P.nmu] - L.smu[0]) : 0;
    return q;
}

// One pass of a tile covers the nb <= P.window bins from wlo on: their edges into sed, their tables zeroed (the
// forwards' sums) or loaded from src (the adjoints' coefficients); a __syncthreads() follows in the kernel.
__device__ __forceinline__ int window_edges(const PParams &P, const PTile &t, int wlo, double *sed, const double *edges)
{
    const int nb = min(P.window, t.bhi - wlo + 1);
    for (int i = threadIdx.x; i <= nb; i += PBLOCK) sed[i] = edges[wlo + i];
    return nb;
}

__device__ __forceinline__ void window_zero(double *tab, int n)
{
    for (int i = threadIdx.x; i < n; i += PBLOCK) tab[i] = 0;
}
__device__ __forceinline__ void window_load(double *tab, int n, const double *src)
{
    for (int i = threadIdx.x; i < n; i += PBLOCK) tab[i] = src[i];
}

// the bin of x, window edges sed[0] <= x < sed[nb], counted from wlo
__device__ __forceinline__ int window_bin(const double *sed, int nb, int wlo, double x, const PGuess &q)
{
    return find_bin(sed, nb, x, guess(x, q.e0, q.inv) - wlo);
}

// the window table tab (n doubles in records of `width`, the count first) into the global sums: contiguous runs of
// doubles, bins that received nothing skipped
__device__ __forceinline__ void window_add(double *sums, const double *tab, int n, int width)
{
    for (int i = threadIdx.x; i < n; i += PBLOCK)
        if (tab[(i / width) * width] != 0) unsafeAtomicAdd(sums + i, tab[i]);
}

// the running sums of one thread for one key (a bin, or a (bin, mu) cell): the LDS atomics of the forwards happen
// once per run of modes with the same key, not once per mode
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
    // the run of `k`: the sums so far go to tab when the key changes
    __device__ __forceinline__ void select(int k, double *tab, int stride)
    {
        if (k != key) {
            flush(tab, stride, stride);
            reset(k);
        }
    }
};

// The adjoints write every element of a tile exactly once.  A tile that spans more bins than a window holds takes one
// pass per window: the pass whose window holds an element's bin writes it, and an element x with no bin at all (outside
// [lo, hi), the edges all passes cover together) is written, as zero, by the first pass.  (corr_vjp_kernel spells
// the same test out: through this function its (r, mu) variant ran 0.8 % slower at 512^3, 1.227 against 1.217 ms.)
__device__ __forceinline__ bool pass_writes_zero(bool first, double x, double lo, double hi)
{
    return first && !(x >= lo && x < hi);
}

// a tile none of whose elements has a bin: put(i0, i1) stores this lane's zero of every row of this wave
template <typename Put> __device__ __forceinline__ void tile_zero(const PTile &t, const PRows &w, Put put)
{
    if (!w.lane_on) return;
    for (int r = w.r0; r < w.r1; r++) {
        int i0, i1;
        row_index(t, r, i0, i1);
        put(i0, i1);
    }
}

// ---- the k side alone (power_kernel and power_vjp_kernel) -----------------------------------------------------------

// A mode of a compressed spectrum stands for itself and its conjugate when its index along the logical last axis is
// neither 0 nor N / 2.  ilast_fixed: that index where the last axis is the lane's (g.alast == 2).
__device__ __forceinline__ bool mode_hermitian(const PParams &P, const PGeom &g, const PTile &t, int64_t ilast_fixed,
                                               int i0, int i1)
{
    bool h = false;
    if (P.hermitian) {
        // (selects, as in tile_begin: t.o[g.alast] would put the tile into scratch memory)
        const int64_t il = g.alast == 2 ? ilast_fixed
                                        : g.start[g.alast] + (g.alast == 0 ? t.o[0] : t.o[1]) + (g.alast == 0 ? i0 : i1);
        h = il != 0 && il != g.nlast / 2;
    }
    return h;
}

// vr, vi over the sinc powers of the mode (s0, s1, s2 in memory order), divided axis by axis in logical order
__device__ __forceinline__ void sinc_divide(const PGeom &g, double s0, double s1, double s2, double &vr, double &vi)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double sp = g.ax[0] == d ? s0 : (g.ax[1] == d ? s1 : s2);
        vr /= sp;
        vi /= sp;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------

// Checks the arguments the forward and the adjoint share and fills the kernel parameters: per_bin / per_cell doubles
// per k bin / (k, mu) cell of the table whose window lives in LDS.  order[m]: the logical axis at memory-order
// position m (axes of extent 1 slowest, then by decreasing stride of a).  *ntiles = 0: nothing to do.
static int power_setup(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a, const int64_t *a_strides,
                       const void *b, const int64_t *b_strides, const int64_t *shape, const int64_t *start,
                       const int64_t *nmesh, const double *boxsize, const double *kedges, const double *muedges,
                       int per_bin, int per_cell, PParams &P, PGeom &g, int64_t *ntiles, size_t *lds)
{
    PMX_REQUIRE(p && ndim >= 1 && ndim <= 3 && a && a_strides && shape && start && nmesh && boxsize && kedges,
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

    P.nk = p->nk;
    P.nmu = p->nmu;
    P.npoles = p->npoles;
    for (int i = 0; i < PMX_POWER_MAX_POLES; i++) P.poles[i] = i < p->npoles ? p->poles[i] : -1;
    P.hermitian = p->hermitian ? 1 : 0;
    P.deconv_pow = p->deconv_pow;
    P.cross = b ? 1 : 0;
    P.volume = p->volume;
    P.s1 = per_bin;
    P.window = lds_window(p->nmu, per_bin, per_cell);
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
    int32_t ax[3];
    axis_order(AXES_UNIT_SLOWEST, sh, sa, ax);
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
    *ntiles = (int64_t)g.nt[0] * g.nt[1] * g.nt[2];
    if (*ntiles == 0 || g.shape[0] * g.shape[1] * g.shape[2] == 0) {
        *ntiles = 0;
        return PMX_OK;
    }
    PMX_REQUIRE(*ntiles < (1ll << 31), PMX_EUNSUPPORTED, "more than 2^31 tiles");
    *lds = sizeof(double) * lds_doubles(p->nmu, per_bin, per_cell, P.window);
    return PMX_OK;
}

// The launch of one of the tile kernels K<T, MU, POLES>: pick(c, m, pl) returns the instance for the canvas type, the
// (k, mu) table and the multipoles; one workgroup per tile.
template <typename Pick, typename... Args>
static int launch_tiles(int32_t elsize, const pmx_power *p, int64_t ntiles, size_t lds, void *stream, Pick pick,
                        Args... args)
{
    with_canvas(elsize, [&](auto c) {
        with_bool(p->nmu > 0, [&](auto m) {
            with_bool(p->npoles > 0, [&](auto pl) {
                pick(c, m, pl)<<<dim3((unsigned)ntiles), PBLOCK, lds, (hipStream_t)stream>>>(args...);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

}  // namespace pmx
