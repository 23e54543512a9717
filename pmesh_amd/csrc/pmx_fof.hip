// pmx_fof.hip — friends-of-friends groups of particles (include/pmesh_amd.h: pmx_fof_cells, pmx_fof_fill, pmx_fof_link,
// pmx_fof_flatten, pmx_fof_minlabel, pmx_fof_group_sums; pmesh_amd/fof.py).
//
// Replaces what a caller of the reference does on the host for a halo catalogue (nbodykit's FOF: a kd-tree over the
// rows copied over PCIe, its merge loop over the ranks, and numpy bincounts for the centres).  The rule — wrapping,
// the friendship test in double with the minimum image, minid — is written down in the header.  The passes:
//   cells_kernel      one lane per row: the wrapped row, its cell, one integer atomic on the cell's count
//   fill_kernel       one lane per row: its slot in cell order (one integer atomic on the cell's cursor), the wrapped
//                     row copied there, so that the link pass reads the rows of a cell from consecutive addresses
//   init_kernel       parent[i] = i (a launch of its own: the link pass reads parents other lanes have not written)
//   link_kernel       one lane per slot: the rows of lower index in the 3^ndim neighbouring cells; friends are united
//                     in a union-find whose only write is an atomic minimum on the slot of a root
//   flatten_kernel    parent[i] = the root of i
//   min_kernel, gather_kernel   the minimum of a value over every component: into the root's slot, then back
//   sums_kernel       per-label sums for the catalogue, equal labels reduced within the wave before the atomics
// Every loop over parents walks strictly decreasing indices (parent[x] <= x always: parents start at x and are only
// lowered), so it ends whatever the other lanes do; no lane waits for a value another lane has to write.  Parent reads
// and updates in link_kernel and flatten_kernel are relaxed agent-scope atomics: a plain load may be served stale from
// another XCD's L2.  A stale parent is still an ancestor (parents only move towards the root), and a root is only ever
// taken for one by the atomic minimum that returns the root's own index.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_cells_dev.h"
#include "pmx_common.h"

namespace pmx {

constexpr int FBLOCK = 256;

template <int NDIM, int PE>
__global__ void __launch_bounds__(FBLOCK) cells_kernel(FGeom g, DVec pos, int64_t n, double *__restrict__ wpos,
                                                       int32_t *__restrict__ cell_of, int32_t *__restrict__ counts,
                                                       int64_t *__restrict__ flagged)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t c = 0;
    bool bad = false;
#pragma unroll
    for (int d = 0; d < NDIM; d++) {
        const double x = pos_get<PE>(pos, i, d);
        bad |= !isfinite(x);
        const double w = fof_wrap(x, g.L[d]);
        wpos[i * NDIM + d] = w;
        c = c * g.nc[d] + fof_cell(g, d, w);
    }
    cell_of[i] = c;
    atomicAdd(&counts[c], 1);
    if (bad) atomicAdd((unsigned long long *)flagged, 1ull);
}

template <int NDIM>
__global__ void __launch_bounds__(FBLOCK) fill_kernel(int64_t n, const double *__restrict__ wpos,
                                                      const int32_t *__restrict__ cell_of,
                                                      const int32_t *__restrict__ cell_start,
                                                      int32_t *__restrict__ cursor, int32_t *__restrict__ order,
                                                      double *__restrict__ spos)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t c = cell_of[i];
    const int64_t slot = (int64_t)cell_start[c] + atomicAdd(&cursor[c], 1);
    if (slot >= n) return;                       // (never, with the counts the starts were made of)
    order[slot] = (int32_t)i;
#pragma unroll
    for (int d = 0; d < NDIM; d++) spos[slot * NDIM + d] = wpos[i * NDIM + d];
}

__global__ void __launch_bounds__(FBLOCK) init_kernel(int64_t n, int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

__device__ __forceinline__ int32_t parent_load(int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the end of the parent chain of x as this lane sees it: strictly decreasing, so it ends
__device__ __forceinline__ int32_t fof_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = parent_load(parent, x);
        if (p >= x) return x;                    // (p == x: parent[x] <= x always)
        x = p;
    }
}

// unite the components of a and b.  max(ra, rb) strictly decreases from one turn to the next: the loop ends.
__device__ __forceinline__ void fof_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        int32_t ra = fof_find(parent, a), rb = fof_find(parent, b);
        if (ra == rb) return;
        if (ra < rb) {
            const int32_t t = ra;
            ra = rb;
            rb = t;
        }
        // ra > rb: rb under ra's slot, if ra still is a root
        const int32_t old = __hip_atomic_fetch_min(parent + ra, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == ra) return;
        // ra had been hooked under old < ra by another lane, and now hangs under min(old, rb): old and rb remain to be
        // united
        a = old;
        b = rb;
    }
}

template <int NDIM>
__global__ void __launch_bounds__(FBLOCK) link_kernel(FGeom g, int64_t n, double b2, const double *__restrict__ spos,
                                                      const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ cell_of,
                                                      const int32_t *__restrict__ cell_start, int32_t *parent)
{
    const int64_t k = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (k >= n) return;
    const int32_t i = order[k];
    if (i < 0 || i >= n) return;                 // (never, with the order fill_kernel left)
    double x[NDIM];
#pragma unroll
    for (int d = 0; d < NDIM; d++) x[d] = spos[k * NDIM + d];
    int32_t c[3];
    fof_cell_axes<NDIM>(g, cell_of[i], c);
    for (int nb = 0; nb < fof_neighbours<NDIM>(); nb++) {
        int32_t cell;
        if (!fof_neighbour<NDIM>(g, c, nb, cell)) continue;
        const int32_t s0 = max(cell_start[cell], 0), s1 = (int32_t)min((int64_t)cell_start[cell + 1], n);
        for (int32_t s = s0; s < s1; s++) {
            const int32_t j = order[s];
            if (j >= i || j < 0) continue;
            double r2 = 0;
#pragma unroll
            for (int d = 0; d < NDIM; d++) {
                const double dx = fof_image(x[d] - spos[(int64_t)s * NDIM + d], g.L[d]);
                r2 += dx * dx;
            }
            if (r2 <= b2) fof_unite(parent, i, j);
        }
    }
}

__global__ void __launch_bounds__(FBLOCK) flatten_kernel(int64_t n, int32_t *parent)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i >= n) return;
    // (the parents other lanes store meanwhile are roots: whichever this lane reads, the chain goes down to the root)
    const int32_t r = fof_find(parent, (int32_t)i);
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(FBLOCK) min_kernel(int64_t n, const int32_t *__restrict__ root,
                                                     const int64_t *__restrict__ val, int64_t *work)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t r = root[i];
    if (r != i && r >= 0 && r < n)
        __hip_atomic_fetch_min((long long *)work + r, (long long)val[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(FBLOCK) gather_kernel(int64_t n, const int32_t *__restrict__ root,
                                                        const int64_t *__restrict__ work, int64_t *__restrict__ val,
                                                        int64_t *__restrict__ changed)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const int32_t r = root[i];
        if (r >= 0 && r < n) {
            const int64_t v = work[r];
            moved = v != val[i];
            if (moved) val[i] = v;
        }
    }
    const unsigned long long m = __ballot(moved);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll(m) - 1))
        atomicAdd((unsigned long long *)changed, (unsigned long long)__popcll(m));
}

// the sum of v over the lanes of `mine` (every lane of the wave takes part; the others add 0)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NDIM, int PE>
__global__ void __launch_bounds__(FBLOCK) sums_kernel(int64_t n, DVec pos, const int64_t *__restrict__ labels,
                                                      DVec mass, DVec vel, const double *__restrict__ ref,
                                                      int64_t ngroups, double L0, double L1, double L2,
                                                      double *__restrict__ out)
{
    constexpr int NCOL = 1 + 2 * NDIM;
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t label = 0;
    if (i < n) {
        label = labels[i];
        if (label < 0 || label > ngroups) label = 0;
    }
    double v[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; c++) v[c] = 0;
    if (label > 0) {
        const double m = mass.data ? mass.get(i, 0) : 1.0;
        v[0] = m;
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            const double L = d == 0 ? L0 : (d == 1 ? L1 : L2);
            const double dx = fof_image(fof_wrap(pos_get<PE>(pos, i, d), L) - fof_wrap(ref[label * NDIM + d], L), L);
            v[1 + d] = m * dx;
            v[1 + NDIM + d] = vel.data ? m * vel.get(i, d) : 0.0;
        }
    }
    // the labels of the wave one after the other (the loop is uniform over the wave): the lanes of the label sum their
    // columns, the first of them adds the sums
    unsigned long long todo = __ballot(label > 0);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        const int64_t lead = __shfl(label, src, 64);
        const bool mine = label == lead;
        todo &= ~__ballot(mine);
#pragma unroll
        for (int c = 0; c < NCOL; c++) {
            const double s = wave_sum(mine ? v[c] : 0.0);
            if (lane == src) atomicAdd(&out[lead * NCOL + c], s);
        }
    }
}

}  // namespace pmx

using namespace pmx;

static inline unsigned fof_grid(int64_t n) { return (unsigned)((n + FBLOCK - 1) / FBLOCK); }

#define FOF_ROWS(n)                                                                                        \
    PMX_REQUIRE((n) >= 0, PMX_EINVAL, "bad arguments");                                                      \
    PMX_REQUIRE((n) <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED, "more than 2^31 - 1 rows: parents are 32-bit")

extern "C" int pmx_fof_cells(int32_t ndim, const pmx_vec *pos, int64_t n, const double *boxsize, const double *origin,
                             const double *inv_side, const int64_t *ncell, int32_t periodic, double *wpos,
                             int32_t *cell_of, int32_t *counts, int64_t *flagged, void *stream)
{
    FGeom g;
    int64_t ncells;
    const int rc = fof_geom(ndim, boxsize, origin, inv_side, ncell, periodic, g, &ncells);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(origin && inv_side, PMX_EINVAL, "bad arguments");
    FOF_ROWS(n);
    if (n == 0) return PMX_OK;
    PMX_REQUIRE(vec_ok(pos) && pos->ncol >= ndim, PMX_EINVAL, "pos must hold ndim float or double columns");
    PMX_REQUIRE(wpos && cell_of && counts && flagged, PMX_EINVAL, "bad arguments");
    const DVec p = dvec(pos);
    hipStream_t st = (hipStream_t)stream;
    with_count<3>(ndim, [&](auto nd) {
        with_elsize(pos->elsize, [&](auto pe) {
            cells_kernel<nd, pe><<<fof_grid(n), FBLOCK, 0, st>>>(g, p, n, wpos, cell_of, counts, flagged);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fof_fill(int32_t ndim, int64_t n, const double *wpos, const int32_t *cell_of,
                            const int32_t *cell_start, int32_t *cursor, int32_t *order, double *spos, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    FOF_ROWS(n);
    if (n == 0) return PMX_OK;
    PMX_REQUIRE(wpos && cell_of && cell_start && cursor && order && spos, PMX_EINVAL, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    with_count<3>(ndim, [&](auto nd) {
        fill_kernel<nd><<<fof_grid(n), FBLOCK, 0, st>>>(n, wpos, cell_of, cell_start, cursor, order, spos);
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fof_link(int32_t ndim, int64_t n, const double *spos, const int32_t *order, const int32_t *cell_of,
                            const int32_t *cell_start, const int64_t *ncell, int32_t periodic, const double *boxsize,
                            double b2, int32_t *parent, void *stream)
{
    FGeom g;
    int64_t ncells;
    const int rc = fof_geom(ndim, boxsize, nullptr, nullptr, ncell, periodic, g, &ncells);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(b2 > 0 && isfinite(b2), PMX_EINVAL, "the linking length must be finite and positive");
    FOF_ROWS(n);
    if (n == 0) return PMX_OK;
    PMX_REQUIRE(spos && order && cell_of && cell_start && parent, PMX_EINVAL, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    init_kernel<<<fof_grid(n), FBLOCK, 0, st>>>(n, parent);
    with_count<3>(ndim, [&](auto nd) {
        link_kernel<nd><<<fof_grid(n), FBLOCK, 0, st>>>(g, n, b2, spos, order, cell_of, cell_start, parent);
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fof_flatten(int64_t n, int32_t *parent, void *stream)
{
    FOF_ROWS(n);
    if (n == 0) return PMX_OK;
    PMX_REQUIRE(parent, PMX_EINVAL, "bad arguments");
    flatten_kernel<<<fof_grid(n), FBLOCK, 0, (hipStream_t)stream>>>(n, parent);
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fof_minlabel(int64_t n, const int32_t *root, int64_t *val, int64_t *work, int64_t *changed,
                                void *stream)
{
    FOF_ROWS(n);
    PMX_REQUIRE(changed, PMX_EINVAL, "bad arguments");
    if (n == 0) return PMX_OK;
    PMX_REQUIRE(root && val && work, PMX_EINVAL, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    PMX_HIP_CHECK(hipMemcpyAsync(work, val, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    min_kernel<<<fof_grid(n), FBLOCK, 0, st>>>(n, root, val, work);
    gather_kernel<<<fof_grid(n), FBLOCK, 0, st>>>(n, root, work, val, changed);
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fof_group_sums(int32_t ndim, int64_t n, const pmx_vec *pos, const int64_t *labels,
                                  const pmx_vec *mass, const pmx_vec *vel, const double *ref, int64_t ngroups,
                                  const double *boxsize, double *out, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    PMX_REQUIRE(n >= 0 && ngroups >= 0 && boxsize, PMX_EINVAL, "bad arguments");
    if (n == 0 || ngroups == 0) return PMX_OK;
    PMX_REQUIRE(vec_ok(pos) && pos->ncol >= ndim, PMX_EINVAL, "pos must hold ndim float or double columns");
    PMX_REQUIRE(labels && ref && out, PMX_EINVAL, "bad arguments");
    const bool has_mass = mass && mass->data, has_vel = vel && vel->data;
    PMX_REQUIRE(!has_mass || vec_ok(mass), PMX_EINVAL, "mass must be float or double");
    PMX_REQUIRE(!has_vel || (vec_ok(vel) && vel->ncol >= ndim), PMX_EINVAL, "vel must hold ndim float or double columns");
    double L[3] = {1, 1, 1};
    for (int d = 0; d < ndim; d++) {
        PMX_REQUIRE(boxsize[d] > 0 && isfinite(boxsize[d]), PMX_EINVAL, "bad boxsize");
        L[d] = boxsize[d];
    }
    PMX_REQUIRE((n + FBLOCK - 1) / FBLOCK < (1ll << 31), PMX_EUNSUPPORTED, "more than 2^31 workgroups");
    const DVec p = dvec(pos), m = dvec(has_mass ? mass : nullptr), v = dvec(has_vel ? vel : nullptr);
    hipStream_t st = (hipStream_t)stream;
    with_count<3>(ndim, [&](auto nd) {
        with_elsize(pos->elsize, [&](auto pe) {
            sums_kernel<nd, pe><<<fof_grid(n), FBLOCK, 0, st>>>(n, p, labels, m, v, ref, ngroups, L[0], L[1], L[2], out);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
