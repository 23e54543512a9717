/*
 * pmesh_amd.h — C ABI of the MI355X-native particle-mesh hot path.
 *
 * This is the drop-in boundary for the PM cycle
 *     decompose -> paint -> r2c -> apply-transfer -> c2r -> readout
 * of MP-Gadget/pmesh.  Every entry point replaces one native interface of the
 * reference (cited per function as file:line relative to the reference tree).
 * The reference's native boundary is per particle (pmesh/_window_imp.h:76-86:
 * pmesh_painter_paint(painter, pos[], weight, hsml) called from a Python-level
 * loop, pmesh/_window.pyx:157-165); a GPU needs the whole particle batch, so
 * the entry points here are the batched form of the same contract.
 *
 * Conventions
 *  - plain C: pointers + sizes, no torch / numpy types.
 *  - all `void*` data pointers are DEVICE pointers (HBM) for the pmx_* library
 *    (libpmesh_amd.so).  The test oracle (oracle/liboracle.so) exports the
 *    same signatures with the prefix pmo_ and HOST pointers.
 *  - strides are in BYTES (as numpy strides; pmesh/_window.pyx:152-154).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every kernel,
 *    copy and fill of an entry is enqueued on that stream, in order, and on no other.
 *    Calls are asynchronous with respect to the host unless stated otherwise.  Stated
 *    otherwise, here in one place (tests/test_streams.py holds both promises for every
 *    entry that takes `stream`):
 *      pmx_whitenoise         waits for the stream before it returns while the master seed stream runs on the host
 *                             (the default, pmx_whitenoise_master(0)): the seed tables it copies are its own.
 *      pmx_binplan_build      waits once in the life of a plan object: a build of 2^16 rows or more with the
 *                             tile-ordered copy left to the library (pmx_binplan_sorted -1) on a plan that has not yet
 *                             measured the coherence of about as many rows reads that measurement back.
 *      first calls            an entry that grows a pooled buffer frees the old one (hipFree waits for the device) and
 *                             allocates: the buffers of a bin plan (pmx_binplan_build, pmx_paint_binned[_defer],
 *                             pmx_readout_binned[_multi], pmx_binplan_order) when the batch or the block outgrows them, the
 *                             chunk tables of pmx_decompose_count / _fill; and the first LDS transform of a length and
 *                             precision on a device (pmx_colfft*, pmx_rowfft*) and the first finite-difference transfer of
 *                             a mesh and box side copy a table from the host synchronously.  Warm, none of them waits.
 *    The entries without a stream (pmx_fft_create / _destroy, pmx_binplan_create / _destroy, pmx_window_set_table and
 *    the settings) are host calls; pmx_window_set_table copies synchronously.  A plan object (pmx_binplan, pmx_fft)
 *    is mutable state: its calls belong on one stream at a time.
 *  - every function returns a pmx_status; pmx_last_error() gives the message.
 */
#ifndef PMESH_AMD_H
#define PMESH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_MAXDIM 3
#define PMX_MAXRANKS 64      /* decomposition targets are kept as a 64-bit mask */
#define PMX_MAXSUPPORT 32    /* same cap as the reference (_window_generics.h:23) */

typedef enum pmx_status {
    PMX_OK = 0,
    PMX_EINVAL = 1,       /* bad argument */
    PMX_EUNSUPPORTED = 2, /* valid in the reference but not built here (yet) */
    PMX_EHIP = 3,         /* HIP runtime error */
    PMX_EFFT = 4,         /* rocFFT error */
    PMX_ENOMEM = 5
} pmx_status;

/* Window kinds on the path (pmesh/_window_imp.h:4-28; window.py:230-255): every kind of the
 * reference's registry, the table-driven ones (lanczos, acg, db / sym wavelets) after
 * pmx_window_set_table. */
typedef enum pmx_window_kind {
    PMX_NEAREST = 0,   /* PMESH_PAINTER_NEAREST   */
    PMX_LINEAR = 1,    /* PMESH_PAINTER_LINEAR    */
    PMX_QUADRATIC = 2, /* PMESH_PAINTER_QUADRATIC */
    PMX_CUBIC = 3,     /* PMESH_PAINTER_CUBIC     */
    PMX_TUNED_NNB = 4, /* PMESH_PAINTER_TUNED_NNB */
    PMX_TUNED_CIC = 5, /* PMESH_PAINTER_TUNED_CIC */
    PMX_TUNED_TSC = 6, /* PMESH_PAINTER_TUNED_TSC */
    PMX_TUNED_PCS = 7, /* PMESH_PAINTER_TUNED_PCS */
    /* table driven (generic path only; need pmx_window_set_table first) */
    PMX_LANCZOS2 = 8, PMX_LANCZOS3 = 9, PMX_LANCZOS4 = 10, PMX_LANCZOS5 = 11, PMX_LANCZOS6 = 12,
    PMX_ACG2 = 13, PMX_ACG3 = 14, PMX_ACG4 = 15, PMX_ACG5 = 16, PMX_ACG6 = 17,
    /* scaling functions of orthonormal wavelets, tabulated on [0, support) (_window_wavelets.h) */
    PMX_DB6 = 18, PMX_DB12 = 19, PMX_DB20 = 20, PMX_SYM6 = 21, PMX_SYM12 = 22, PMX_SYM20 = 23
} pmx_window_kind;

/* The geometric part of `struct PMeshPainter` (pmesh/_window_imp.h:48-62):
 * window, affine transform, periodicity and the canvas block it addresses. */
typedef struct pmx_painter {
    int32_t kind;          /* pmx_window_kind */
    int32_t support;       /* <= 0: native support (window_info_init, _window_imp.c:24-47) */
    int32_t ndim;          /* 1..3 */
    int32_t canvas_elsize; /* 4 (float) or 8 (double) */
    int32_t order[PMX_MAXDIM];   /* 0 = window, 1 = derivative along that axis */
    int32_t _pad;
    double scale[PMX_MAXDIM];     /* grid = pos * scale + translate (no FMA) */
    double translate[PMX_MAXDIM];
    int64_t period[PMX_MAXDIM];   /* Nmesh; 0 = non periodic */
    int64_t size[PMX_MAXDIM];     /* extent of the local canvas block */
    int64_t strides[PMX_MAXDIM];  /* canvas strides in bytes */
} pmx_painter;

/* The same for meshes of 4 to PMX_MAXDIM_ND dimensions (the reference's painter takes up to 32, _window_imp.h:50-60;
 * ParticleMesh.reshape(Nmesh=[8, 8, 8, 8]), pmesh/tests/test_pm.py:381-384): a struct of its own, because pmx_painter
 * travels by value to the hot kernels of the 3-d path and every element costs them scalar registers.  Served by the
 * generic per-particle kernels only (pmx_paint_nd / pmx_readout_nd; no tuned, no tile-binned path). */
#define PMX_MAXDIM_ND 8
typedef struct pmx_painter_nd {
    int32_t kind;          /* pmx_window_kind */
    int32_t support;       /* <= 0: native support */
    int32_t ndim;          /* 1..PMX_MAXDIM_ND */
    int32_t canvas_elsize; /* 4 (float) or 8 (double) */
    int32_t order[PMX_MAXDIM_ND];
    double scale[PMX_MAXDIM_ND];
    double translate[PMX_MAXDIM_ND];
    int64_t period[PMX_MAXDIM_ND];
    int64_t size[PMX_MAXDIM_ND];
    int64_t strides[PMX_MAXDIM_ND];
} pmx_painter_nd;

/* A strided per-particle column set (numpy view semantics): element (i, c) is
 * at data + i*stride0 + c*stride1 and is a float (elsize 4) or double (8).
 * Mirrors the fused postype/masstype/hsmltype arguments of _window.pyx:6-16. */
typedef struct pmx_vec {
    void *data;      /* NULL = absent */
    int32_t elsize;  /* 4 or 8 */
    int32_t ncol;
    int64_t stride0; /* bytes between particles (0 broadcasts one row) */
    int64_t stride1; /* bytes between columns */
} pmx_vec;

const char *pmx_last_error(void);
int pmx_version(void);
/* the compiler line libpmesh_amd.so was built with (csrc/Makefile); a build that contains wrong-result timing
 * experiments carries -DPMX_EXPERIMENT there and bench.py refuses to report numbers for it */
const char *pmx_build_flags(void);
/* number of visible HIP devices (0 if none); never throws */
int pmx_device_count(void);

/* ---- window metadata ---------------------------------------------------- */
/* pmesh_painter_init + pmesh_window_info_init (_window_imp.c:24-47, 246-459):
 * native support and effective integer support of (kind, support). */
int pmx_window_info(int32_t kind, int32_t support, int32_t *nativesupport, int32_t *eff_support);
/* Register the lookup table of a table-driven kind on the current device (the reference
 * compiles them in: pmesh/_window_lanczos.h, _window_acg.h; `_<name>_kernel/_diff` there):
 * n values on [0, (n-1)*step], HOST array, linear interpolation.  Once per device and kind. */
int pmx_window_set_table(int32_t kind, const double *values, int32_t n, double step);
/* pmesh_painter_get_fwindow (_window_imp.c:473-485) for n circular
 * frequencies; HOST arrays (tiny, init-time). */
int pmx_fwindow(int32_t kind, int32_t support, const double *w, int64_t n, double *out);

/* ---- paint / readout ---------------------------------------------------- */
/* Batched form of pmesh_painter_paint over the Cython loop _window.pyx:128-165:
 *   for i < npart: canvas[cells of window at pos[i]] += mass[i] * W(...)
 * mass == NULL or mass->data == NULL means every particle has `mass_scalar`
 * (the 0-stride broadcast of window.py:6-16,146).  hsml NULL = 1.0.
 * Cells outside the local block after periodic wrapping are dropped
 * (_window_generics.h:144-167). Accumulates into the canvas (window.py:113). */
int pmx_paint(const pmx_painter *p, void *canvas, const pmx_vec *pos, const pmx_vec *mass,
              double mass_scalar, const pmx_vec *hsml, int64_t npart, void *stream);

/* Batched form of pmesh_painter_readout (_window.pyx:167-205):
 *   out[i] = sum over window cells canvas[cell] * W(...), in the reference's
 * lexicographic cell order, stored as float or double per out->elsize. */
int pmx_readout(const pmx_painter *p, const void *canvas, const pmx_vec *pos, const pmx_vec *hsml,
                const pmx_vec *out, int64_t npart, void *stream);
/* pmx_paint / pmx_readout for meshes of up to PMX_MAXDIM_ND dimensions (_generic_paint / _generic_readout,
 * _window_generics.h:4-142, with _fill_k, _window_imp.c:50-83: any kind, any integer support <= PMX_MAXSUPPORT,
 * per-particle hsml).  For ndim <= 3 the same numbers as the generic path of pmx_paint / pmx_readout. */
int pmx_paint_nd(const pmx_painter_nd *p, void *canvas, const pmx_vec *pos, const pmx_vec *mass,
                 double mass_scalar, const pmx_vec *hsml, int64_t npart, void *stream);
int pmx_readout_nd(const pmx_painter_nd *p, const void *canvas, const pmx_vec *pos, const pmx_vec *hsml,
                   const pmx_vec *out, int64_t npart, void *stream);

/* ---- tile-binned paint / readout (device-side acceleration structure) ---- */
/* A bin plan orders the particles of one batch by mesh tile (an index list per
 * tile; positions are not copied) so that paint accumulates each tile in LDS
 * and writes it with plain stores, and readout gathers from an LDS-staged tile.
 * 3-d meshes, tuned windows (NNB/CIC/TSC/PCS) at native support, no hsml.
 * Results: readout is bit-identical to pmx_readout; paint equals pmx_paint up
 * to the order of floating-point additions into a cell.  One plan serves any
 * number of paint/readout calls on the same positions and geometry (the PM
 * cycle paints and reads out at the same positions). */
typedef struct pmx_binplan pmx_binplan;
int pmx_binplan_create(pmx_binplan **plan);
int pmx_binplan_destroy(pmx_binplan *plan);
/* Which kernels the next builds of this plan serve: 0 / -1 (default) = tile form (one workgroup
 * accumulates a tile of 8 x 16 x 32 cells in LDS), 2 = tiles with the chunk form of the single-pass
 * rebuild (what plans with a tile-ordered copy use; a test hook).  1 was the walk form of rounds
 * 2-3 (a measured alternative that was no faster on MI355X; removed): PMX_EUNSUPPORTED.
 * Same results in every form (readout bit-identical, paint up to the order of the additions into
 * a cell). */
int pmx_binplan_configure(pmx_binplan *plan, int32_t form);
/* Arithmetic of pmx_readout_binned.  The cell indices of a particle are always the reference's bit for bit
 * (floor(pos * scale + translate) in double precision without FMA, _window_tuned_*.h).  on = 1: the weights and
 * the sum are also formed operation by operation as the reference does (_window_generics.h:213-242): results
 * bit-identical to pmx_readout and to the CPU reference.  on = 0 (default): the weights are the same polynomials
 * evaluated in one offset with fused multiply-adds, and the S^3 products are summed as nested FMAs in the type of
 * the canvas — a third of the instructions; results within 1e-14 (double canvas) / 1e-6 (float canvas) of the
 * exact form relative to the sum of |weight x cell|, inside the tolerance the parity tests allow for values. */
int pmx_binplan_exact(pmx_binplan *plan, int32_t on);
/* Deterministic paint (the reference's scatter is a serial loop, pmesh/_window.pyx:157-165: the same call gives
 * the same bits).  on = 1: pmx_paint_binned accumulates every cell as a 64-bit integer in units of 2^-f — the
 * LDS regions, the halos between tiles (integer atomics on a dense int64 copy of the block) and the pieces of
 * crowded tiles — with one f for the batch (from the largest tile population and the largest |mass|), and
 * rounds once into the caller's canvas: independent of the order in which anything arrives, run to run and
 * whatever the order of the rows.  Within 2^-f (<= 2^-50 x the largest |mass| x tile population / 2^11) per
 * contribution of the reference's sum.  Default 0: S >= 3 windows still accumulate their LDS regions in fixed
 * point (it is the faster form), the halos are merged with floating-point atomics. */
int pmx_binplan_deterministic(pmx_binplan *plan, int32_t on);
/* The fixed-point regions of pmx_paint_binned (S >= 3 windows, deterministic paint) take one scale 2^-f per
 * z segment from the largest |mass| of a per-particle mass array, and must know that every mass is finite and
 * that the masses do not span more than 2^20 (a batch that does — or that holds a NaN / Inf — is painted by the
 * floating-point form of the same kernels, exactly as in round 2; see INTEGRATION.md section 1 for the error
 * model).  By default a reduction kernel in front of every paint finds out (one read of the masses).
 * pmx_mass_stats runs that reduction on its own: stats = 4 doubles of device memory (contents opaque);
 * pmx_binplan_mass_stats hands them to the NEXT pmx_paint_binned of the plan, which then skips its own pass
 * (a time-stepping caller computes them once per mass array).  stats = NULL: back to the default. */
int pmx_mass_stats(const pmx_vec *mass, int64_t n, double *stats, void *stream);
int pmx_binplan_mass_stats(pmx_binplan *plan, const double *stats);
/* Rows without spatial coherence (catalogues in file order, shuffled sets) make every access
 * through the index list a sector of its own.  A plan can instead carry a copy of the positions
 * in tile order (one gather per build): paint and readout stream it, readout writes its results
 * in tile order and pulls them back through the inverse list.  pref: -1 (default) = decided by
 * every build of a geometry from the measured coherence of the row order: a plan without the
 * copy takes it above PMX_SORTED_TAKE_BREAKS changes of tile per 64 consecutive rows, a plan
 * with it gives it up below PMX_SORTED_DROP_BREAKS (two thresholds, so that position sets on
 * either side of one do not restart the plan every step; lattice order shows a handful of
 * breaks, random order 63), 0 = never, 1 = always, -2 = leave unchanged.
 * is_sorted (optional): whether the plan as built carries the copy.  Results do not depend on it
 * (readout bit-identical, paint up to the order of the additions). */
#define PMX_SORTED_TAKE_BREAKS 61.5
#define PMX_SORTED_DROP_BREAKS 58.0
int pmx_binplan_sorted(pmx_binplan *plan, int32_t pref, int32_t *is_sorted);
/* How many builds of this plan so far found the slot ranges of their previous build too small
 * (particles moved a lot) and fell back to the exact two-pass build on the device.  Host
 * counter, written by the device: exact once the stream has been synchronised. */
int pmx_binplan_overflows(pmx_binplan *plan, uint32_t *count);
/* How many particles the tile kernels of this plan have skipped so far because their position no longer lay in
 * the region of the tile their list entry names: the plan was built for other positions — rows rewritten in
 * place without the caller's cache noticing (the reference has no such state: it re-reads every position on
 * every call, pm.py:1795-1869).  Blocks that are the whole periodic mesh cannot tell (a particle's cell modulo
 * the tile is always inside: its mass lands in the wrong cell of the right tile).  Host counter written by the
 * device: exact once the stream has been synchronised; 0 for every correct use. */
int pmx_binplan_stale(pmx_binplan *plan, uint32_t *count);
/* [r5] builds of this plan so far with npart > 0: in ONE pass into the slot ranges of the build before (same geometry,
 * a particle count within an eighth of the previous one: a time-stepping caller, also one whose particles migrate
 * between ranks) / in two passes (the first build, another geometry or count, the back-off after an overflow). */
int pmx_binplan_builds(pmx_binplan *plan, uint32_t *single_pass, uint32_t *two_pass);
/* Which form the plan is in now: in_entry_form = 1 while its last build is in the block-entry form (32-row blocks and
 * a mask per tile; 0 once a consumer of the index list has turned it into the list), drops = the builds of its current
 * history that gave the entry form up (from two on the plan keeps the list).  Host state only: no synchronisation. */
int pmx_binplan_blocks(pmx_binplan *plan, int32_t *in_entry_form, uint32_t *drops);
/* [r6] The order of the rows that a built plan holds, for the caller: order[k] (npart int64 of device memory) = the row that
 * stands k-th when the rows are taken tile by tile — inside a tile in the order of the plan's list, which is not that
 * of the rows and changes from build to build (tests/stream_cases.py: TileOrder) — and the rows that touch no local cell
 * last.  A time-stepping caller re-sorts its particle arrays with it every few steps
 * (ParticleMesh.tile_order; the reference has no counterpart): position gathers and result stores of the tile kernels
 * then touch whole lines again, whatever the flow has done to the order the particles were made in. */
int pmx_binplan_order(pmx_binplan *plan, int64_t *order, void *stream);
/* PMX_OK if (painter, npart) can use the binned kernels */
int pmx_binplan_supported(const pmx_painter *p, int64_t npart);
/* bin the batch: tile id + slot per particle, per-tile counts, scan, index lists */
int pmx_binplan_build(pmx_binplan *plan, const pmx_painter *p, const pmx_vec *pos, int64_t npart,
                      void *stream);
/* overwrite != 0: the canvas content is ignored and every cell of the block is
 * written (paint with hold=False without a separate zero fill, pm.py:1852-1853) */
int pmx_paint_binned(pmx_binplan *plan, const pmx_painter *p, void *canvas, const pmx_vec *pos,
                     const pmx_vec *mass, double mass_scalar, int32_t overwrite, void *stream);
int pmx_readout_binned(pmx_binplan *plan, const pmx_painter *p, const void *canvas,
                       const pmx_vec *pos, const pmx_vec *out, void *stream);
/* [r6] The readout of up to PMX_MAXFIELDS canvases of one block geometry (same painter) at the same positions, the results
 * side by side in the rows of `out`: out(i, f) = canvas f at x_i (`out`: ncol >= ncanvas, any stride0 / stride1) — the
 * three force components of a PM step written once per row (the reference's caller fills F[..., d] column by column,
 * examples/nbody.py:214-216; a column at a time every 64-byte piece of F goes to memory and back three times).  Serves
 * what the default path of pmx_readout_binned serves (relaxed arithmetic, plans without the tile-ordered copy, dense rows
 * of three positions); PMX_EUNSUPPORTED otherwise — the caller then reads the canvases one by one. */
#define PMX_MAXFIELDS 4
int pmx_readout_binned_multi(pmx_binplan *plan, const pmx_painter *p, const void *const *canvases, int32_t ncanvas,
                             const pmx_vec *pos, const pmx_vec *out, void *stream);
/* [r4] The halo merge of a paint left to its consumer.  pmx_paint_binned ends with a pass that adds the staged
 * halos of all tiles (the cells of a tile's region beyond its own box) to their owners with atomics: a
 * read-modify-write of a quarter (CIC) to two thirds (PCS) of the mesh on top of the paint itself.  In the PM cycle
 * the next reader of the mesh is the forward row pass of r2c (pm.py:1795-1869 -> pm.py:655-694), which can add the
 * staged values while it loads the rows: no pass of their own, no atomics.
 * pmx_paint_binned_defer : as pmx_paint_binned; *deferred = 1 if the merge was left out (axes 1 and 2 whole and
 *                          periodic; axis 0 the same — one rank's mesh — or [r5] a block of planes of a larger
 *                          period, a slab rank of domain.py:561-652; overwrite != 0, not deterministic, a row
 *                          length pmx_rowfft_halo gathers for), else 0
 *                          and the call is pmx_paint_binned.  While a plan holds staged halos it refuses to build or
 *                          paint (PMX_EINVAL): one of the next two calls comes first.
 * pmx_halo_merge         : the merge pmx_paint_binned would have run (no-op if nothing is staged).
 * pmx_rowfft_halo        : pmx_rowfft (forward) on rows [x0 * rows_per_plane, ...) of the painted canvas, the staged
 *                          halos added to every row as it is loaded; last != 0 releases the plan (the caller has
 *                          transformed every plane).  Values equal pmx_halo_merge + pmx_rowfft up to the order of
 *                          the additions into a cell. */
int pmx_paint_binned_defer(pmx_binplan *plan, const pmx_painter *p, void *canvas, const pmx_vec *pos,
                           const pmx_vec *mass, double mass_scalar, int32_t overwrite, int32_t *deferred,
                           void *stream);
int pmx_halo_merge(pmx_binplan *plan, const pmx_painter *p, void *canvas, void *stream);
/* what pmx_rowfft_halo reads: the staging buffer of the plan's last deferred paint (elements of the canvas type,
 * ntiles x the halo cells of a tile region in the compact numbering of csrc/pmx_binplan.h), the window support S and
 * nt[4]: the tiles per axis, then the plane of tile space the block starts at along axis 0 (0: one rank's whole mesh;
 * S - 1: a slab rank's block of planes); PMX_EINVAL unless `canvas` / `elsize` are those of that paint.  consume != 0 releases the
 * plan (the staged values are moot: the canvas is gone or about to be overwritten as a whole). */
int pmx_binplan_halo_source(pmx_binplan *plan, const void *canvas, int32_t elsize, const void **halo,
                            int32_t *S, int32_t *nt, int32_t consume);
int pmx_rowfft_halo_supported(int64_t n, int32_t elsize);
int pmx_rowfft_halo(int32_t elsize, void *data, void *dst, int64_t nrows, int64_t n, int64_t pitch, double scale,
                    int64_t rows_per_plane, int64_t plane_pitch, pmx_binplan *plan, const void *canvas,
                    int64_t x0, int32_t last, void *stream);      /* dst: NULL or data = in place, else as pmx_rowfft_to */

/* ---- domain decomposition (pmesh/domain.py:561-652 + _domain.pyx:9-122) -- */
typedef struct pmx_grid {
    int32_t ndim;
    int32_t periodic;
    int32_t nranks;                 /* size of the communicator */
    int32_t shape[PMX_MAXDIM];      /* domains per axis */
    const double *edges[PMX_MAXDIM];/* shape[d]+1 doubles each */
    const int32_t *assign;          /* DomainAssign[prod(shape)]        */
    const int16_t *degenerate;      /* DomainDegenerate[prod(shape)]    */
} pmx_grid;

/* Pass 1 (domain.py:605-636, gridnd_fill mode 0): per particle the set of
 * target ranks within +-smoothing of scale*pos, as a bit mask, and the number
 * of particles per rank.  masks: npart uint64 (out); counts: nranks int64 (out). */
int pmx_decompose_count(const pmx_grid *g, const pmx_vec *pos, const double *scale,
                        const double *smoothing, int64_t npart, uint64_t *masks,
                        int64_t *counts, void *stream);
/* Pass 2 (gridnd_fill mode 1, _domain.pyx:45-51,120-121): rank-major, stable
 * list of particle indices.  offsets: nranks int64 exclusive prefix of counts;
 * indices: sum(counts) integers of index_elsize (4 or 8) bytes. */
int pmx_decompose_fill(int32_t nranks, const uint64_t *masks, int64_t npart,
                       const int64_t *offsets, void *indices, int32_t index_elsize,
                       void *stream);

/* Layout.exchange pack (domain.py:188 `data.take(indices)`): dst row j = src row indices[j]. */
int pmx_take_rows(const void *src, int64_t src_stride0, int64_t row_bytes, const void *indices,
                  int32_t index_elsize, int64_t nrows, void *dst, void *stream);
/* The same into rows `dst_stride` bytes apart: one column of a row that packs several arrays side by side — what
 * Layout.exchange(pack=True) ships (domain.py:161-166, pack_arrays 59-80) — written where it travels from, without
 * gathering the columns one by one and concatenating them.  indices = NULL: dst row j = src row j (a column taken
 * out of packed rows on the receiving side). */
int pmx_pack_rows(const void *src, int64_t src_stride0, int64_t row_bytes, const void *indices,
                  int32_t index_elsize, int64_t nrows, void *dst, int64_t dst_stride, void *stream);
/* Layout.gather mode='sum' (domain.py:294-295, bincountv 26-48):
 * out[i*ncol + c] = sum over j with indices[j] == i of values[j*ncol + c], for all
 * i < nout (rows that receive nothing become 0, as numpy.bincount does).
 * nout = 0: `out` is not cleared first — the rows are added into what it already holds. */
int pmx_scatter_add(const void *values, int32_t elsize, int32_t ncol, const void *indices,
                    int32_t index_elsize, int64_t nrows, void *out, int64_t nout, void *stream);

/* closed-form transfer functions T(k); see pmx_apply_transfer below */
typedef struct pmx_transfer {
    double amplitude;     /* real prefactor */
    int32_t laplace_pow;  /* multiply by (k^2)^laplace_pow, k^2(0) := 1 (nbody.py:156-157); 0 = off */
    int32_t grad_dir;     /* -1 = off; else multiply by i * D(k_dir) */
    int32_t grad_kind;    /* 0: D = k (dx1_transfer nbody.py:154-160);
                             1: D = (8 sin w - sin 2w)/(6 C), w = k C, C = L/N (force_transfer 162-171) */
    int32_t deconv_pow;   /* divide by prod_d sinc(w_d/2)^deconv_pow (window.py:65-80); 0 = off */
    double gauss_r;       /* multiply by exp(-0.5 k^2 r^2) (lowpass_transfer nbody.py:177-181); 0 = off */
} pmx_transfer;

/* ---- FFT (replaces pfft.Plan / plan.execute, pm.py:1429-1434, 689, 1017) -- */
typedef enum pmx_fft_kind { PMX_FFT_R2C = 0, PMX_FFT_C2R = 1, PMX_FFT_C2C_FWD = 2, PMX_FFT_C2C_BWD = 3 } pmx_fft_kind;
typedef struct pmx_fft pmx_fft;
/* A batched strided transform of rank `ndim` over lengths n[] (C order, last
 * axis fastest; for R2C/C2R the real lengths).  Strides/dists in ELEMENTS of
 * the respective side (real elements on the real side, complex on the complex
 * side).  `scale` multiplies the output (r2c carries 1/prod(Nmesh), pm.py:692). */
int pmx_fft_create(pmx_fft **plan, int32_t kind, int32_t elsize, int32_t ndim, const int64_t *n,
                   const int64_t *istride, int64_t idist, const int64_t *ostride, int64_t odist,
                   int64_t batch, double scale, int32_t inplace);
int pmx_fft_execute(pmx_fft *plan, void *in, void *out, void *stream);
int pmx_fft_destroy(pmx_fft *plan);

/* Batched strided ("column") complex FFT, in place, lengths 2^k in 64..2048, 3 * 2^k in 192..1536 and 5 * 2^k in 320..1280, with the
 * columns resident in LDS (csrc/pmx_colfft.hip): the passes of a 3-d transform along the
 * non-contiguous axes.  `data` is an (A, N, B) complex array in C order; the transform runs
 * along the middle axis.  inverse = 0: exp(-i k x); 1: exp(+i k x); unnormalised, the result
 * is multiplied by `scale`.  transfer != NULL fuses ComplexField.apply (pm.py:1047-1070)
 * into the load of the axis-0 pass: A must be 1, B = n1*n2, element (i0, i1, i2) of the
 * local block starting at global index start[] is multiplied by T(k) first (closed forms
 * without transcendentals only: laplace_pow in -1..1, spectral gradient).
 * a_stride / n_stride (complex elements, 0 = dense): stride between successive a (>= N*B) and,
 * for A == 1, between successive lines n (>= B) — the padded plane stride of the one-rank
 * complex layout. */
int pmx_colfft_supported(int64_t n, int32_t elsize);
int pmx_colfft(int32_t elsize, int32_t inverse, void *data, int64_t A, int64_t N, int64_t B,
               double scale, const pmx_transfer *transfer, int64_t n1, int64_t n2, const int64_t *start,
               const int64_t *nmesh, const double *boxsize, int64_t a_stride, int64_t n_stride,
               void *stream);

/* The axis-1 column pass of a slab-decomposed transform fused with the pack / unpack that
 * brackets PFFT's global transpose (what pmx_slab_pack does, for equal power-of-two ranges):
 * inverse = 0: src plain (A, N, B) -> dst "split": block r = lines [r*nsplit, (r+1)*nsplit)
 * as one contiguous (A, nsplit, B) array, i.e. the all-to-all send buffer; inverse = 1: src
 * split (the receive buffer) -> dst plain.  Out of place; unnormalised, times `scale`.
 * plain_pitch: elements per line of the plain side (>= B; 0 = B): the slab layout keeps its
 * real-side rows on 128-byte boundaries while the wire format stays dense. */
int pmx_colfft_split(int32_t elsize, int32_t inverse, const void *src, void *dst, int64_t A, int64_t N,
                     int64_t B, int64_t nsplit, double scale, int64_t plain_pitch, void *stream);

/* r2c -> transfer -> c2r back to back (what a PM force step does with every density field): the last forward
 * pass and the first inverse pass run along the same axis and are one kernel — forward column transform, times
 * `scale` (the forward normalisation), times the transfer function (t != NULL, as in pmx_colfft), inverse column
 * transform, the column resident in LDS — one sweep of the array instead of two, bit-identical to
 * pmx_colfft(inverse = 0, scale) followed by pmx_colfft(inverse = 1, t).  In place on the (N, B) block at
 * n_stride elements per line (0 = B).  PFFT has no such fusion (pm.py:689, 1017 are two separate executes). */
int pmx_colfft_roundtrip_supported(int64_t n, int32_t elsize);
int pmx_colfft_roundtrip(int32_t elsize, void *data, int64_t N, int64_t B, double scale,
                         const pmx_transfer *transfer, int64_t n1, int64_t n2, const int64_t *start,
                         const int64_t *nmesh, const double *boxsize, int64_t n_stride, void *stream);

/* Scheduling of the column passes whose tile fills a compute unit (N = 1024 in both precisions, 768 / 640 in double).
 * persistent = 1 (default): one workgroup per CU walks a fixed share of the tiles and prefetches its next one —
 * the faster form when the GPU is the kernel's alone.  persistent = 0: one workgroup per tile, placed by the hardware
 * as CUs become free — what a process should choose whose transforms overlap with collectives (RCCL's kernels hold
 * CUs for the length of a transfer; a persistent workgroup that cannot be placed beside them starts when another has
 * finished its whole share).  Process-wide; the host side selects 0 for plans on more than one rank.  No PFFT
 * counterpart (pfft.Plan has no such knob). */
int pmx_colfft_configure(int32_t persistent);

/* The axis-1 pass of a pencil transform (PFFT's 2-d process mesh, pm.py:1417-1434) between its two
 * global transposes: src is the (A, N, B) array cut into ranges of nsplit_in lines (the receive
 * buffer of one all-to-all), dst the same array cut into ranges of nsplit_out lines (the send
 * buffer of the other); 0 = plain dense.  Replaces two pmx_slab_pack sweeps around pmx_colfft.
 * nsplit: 0 or a power of two dividing N.  src and dst must not overlap. */
int pmx_colfft_resplit(int32_t elsize, int32_t inverse, const void *src, void *dst, int64_t A, int64_t N,
                       int64_t B, int64_t nsplit_in, int64_t nsplit_out, double scale, void *stream);

/* The axis-0 pass on one chunk [coff, coff + cw) of the last axis of the (N, n1, pitch) block
 * `full` (pipelined slab transposes: the all-to-all of one chunk overlaps the passes of its
 * neighbours; PFFT has no such overlap).  `chunk` is the dense (N, n1, cw) buffer the
 * all-to-all delivers or takes.  to_full = 1: transform `chunk`, scatter into `full`;
 * to_full = 0: gather the chunk's columns from `full` (optionally times the transfer function,
 * as in pmx_colfft; start[] = global start of `full`), transform, write `chunk`. */
int pmx_colfft_chunk(int32_t elsize, int32_t inverse, void *chunk, void *full, int64_t N, int64_t n1,
                     int64_t cw, int64_t pitch, int64_t coff, int32_t to_full, double scale,
                     const pmx_transfer *transfer, const int64_t *start, const int64_t *nmesh,
                     const double *boxsize, void *stream);

/* Real <-> half-complex transform along the contiguous axis, in place, with the rows
 * resident in LDS (csrc/pmx_colfft.hip): `nrows` rows of n reals (n a power of two in
 * 128..2048, or 384 / 768 / 1536 / 640 / 1280) at a pitch of `pitch` complex elements <-> n/2+1 modes.  inverse = 0: r2c,
 * 1: c2r; unnormalised, times `scale`.  rows_per_plane > 0: row r starts at
 * (r / rows_per_plane) * plane_pitch + (r % rows_per_plane) * pitch complex elements (padded
 * plane stride; rows_per_plane a multiple of 8 (f8) / 16 (f4)); 0: r * pitch. */
int pmx_rowfft_supported(int64_t n, int32_t elsize);
int pmx_rowfft(int32_t elsize, int32_t inverse, void *data, int64_t nrows, int64_t n, int64_t pitch,
               double scale, int64_t rows_per_plane, int64_t plane_pitch, void *stream);
/* [r4] The same passes from `src` into `dst` (same layout, distinct buffers): the first pass of a transform whose
 * caller keeps its input — r2c() / c2r() with out=None, the reference's default (pm.py:655-694, 987-1019: PFFT plans
 * built out of place) — reads the input and writes the result buffer; the remaining passes run in place there.
 * Replaces a copy of the whole array in front of an in-place transform (and, for c2r(transfer=...), a separate
 * transfer kernel: the transfer rides on this pass as in pmx_colfft). */
int pmx_rowfft_to(int32_t elsize, int32_t inverse, const void *src, void *dst, int64_t nrows, int64_t n,
                  int64_t pitch, double scale, int64_t rows_per_plane, int64_t plane_pitch, void *stream);
int pmx_colfft_to(int32_t elsize, int32_t inverse, const void *src, void *dst, int64_t A, int64_t N, int64_t B,
                  double scale, const pmx_transfer *transfer, int64_t n1, int64_t n2, const int64_t *start,
                  const int64_t *nmesh, const double *boxsize, int64_t a_stride, int64_t n_stride, void *stream);

/* [r6] The row pass of a pencil transform (PFFT's 2-d process mesh, pm.py:1417-1434) with the last-axis split of its
 * first global transpose on it: inverse = 0: src = nrows rows of n reals (row pitch `pitch` complex elements) -> dst =
 * the n/2 + 1 modes of every row in nparts blocks, block q = the modes [offsets[q], offsets[q + 1]) of all rows as one
 * dense (nrows, offsets[q + 1] - offsets[q]) array at element nrows * offsets[q] — the send buffer of the all-to-all
 * over the row group; inverse = 1: src = those blocks (the receive buffer) -> dst = rows of n reals.  Out of place.
 * Replaces the pmx_slab_pack / pmx_slab_unpack sweep (n0 = nrows, n1 = n/2 + 1, n2 = 1) next to pmx_rowfft; same
 * values.  Built for every length of pmx_rowfft and nparts <= PMX_MAXSEG (offsets: host, nparts + 1 entries from 0
 * to n/2 + 1, not decreasing — empty blocks are allowed). */
#define PMX_MAXSEG 16
int pmx_rowfft_split_supported(int64_t n, int32_t elsize, int32_t nparts);
int pmx_rowfft_split(int32_t elsize, int32_t inverse, const void *src, void *dst, int64_t nrows, int64_t n,
                     int64_t pitch, double scale, const int64_t *offsets, int32_t nparts, void *stream);

/* Local transpose next to the all-to-all of a distributed FFT (PFFT's global transpose).
 * pmx_slab_pack  : src (n0, n1, n2) C order -> nparts contiguous blocks, block r = (n0,
 *                  n1 range [n1_offsets[r], n1_offsets[r+1]), n2): the send buffer of an
 *                  all-to-all that redistributes axis 1.
 * pmx_slab_unpack: the inverse (blocks -> (n0, n1, n2)): what the reverse all-to-all delivers.
 * The blocks an all-to-all delivers for axis 0 are row ranges of the destination array
 * and need no kernel.  Elements are `elbytes` wide (8 = complex64, 16 = complex128). */
int pmx_slab_pack(const void *src, void *dst, int64_t n0, int64_t n1, int64_t n2,
                  const int64_t *n1_offsets /* host, nparts+1 */, int32_t nparts, int32_t elbytes,
                  void *stream);
int pmx_slab_unpack(const void *src, void *dst, int64_t n0, int64_t n1, int64_t n2,
                    const int64_t *n1_offsets /* host, nparts+1 */, int32_t nparts, int32_t elbytes,
                    void *stream);

/* ---- apply-transfer (Field.apply, pm.py:617-648, with the transfer functions
 * of examples/nbody.py:154-181 and pmesh/transfer.py fused) ---------------- */

/* out[m] = T(k(m)) * in[m] over a local complex block of logical shape
 * shape[0..ndim) starting at global index start[], with byte strides; k_d =
 * 2 pi / L_d * (i - N_d [i >= N_d/2]) (pm.py:1200-1226: Nyquist negative).
 * in may equal out.  elsize = 4 (complex64) or 8 (complex128) per component. */
int pmx_apply_transfer(const pmx_transfer *t, int32_t ndim, int32_t elsize, const void *in,
                       const int64_t *in_strides, void *out, const int64_t *out_strides,
                       const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                       const double *boxsize, void *stream);

/* ---- binned power spectrum (what a caller measures on a painted density: nbodykit's FFTPower; the reference's
 * TransferFunction.PowerSpectrum, pmesh/transfer.py:133-181, a slab loop of digitize + bincount) ------------------ */

#define PMX_POWER_MAX_KBINS (1 << 20)  /* k bins: any number up to this; a tile takes its bins in windows (LDS) */
#define PMX_POWER_MAX_MUBINS 64        /* mu bins of the (k, mu) table */
#define PMX_POWER_MAX_POLES 5          /* multipoles per call */
#define PMX_POWER_MAX_ELL 8            /* highest multipole order */

typedef struct pmx_power {
    int32_t nk;                        /* k bins: kedges holds nk + 1 strictly increasing values */
    int32_t nmu;                       /* 0: no (k, mu) table; else muedges holds nmu + 1 increasing values in [-1, 1] */
    int32_t npoles;                    /* 0 .. PMX_POWER_MAX_POLES */
    int32_t poles[PMX_POWER_MAX_POLES];/* their orders ell, 0 .. PMX_POWER_MAX_ELL */
    int32_t hermitian;                 /* 1: a compressed (r2c) half spectrum — see below */
    int32_t deconv_pow;                /* divide v by prod_d sinc(w_d/2)^deconv_pow (as pmx_apply_transfer); 0 = off */
    double volume;                     /* V = prod BoxSize */
    double los[3];                     /* unit line of sight (mu); logical axis order */
} pmx_power;

/* Adds the binned sums of the local complex block a (and b; b = NULL: b = a) into `acc`, a device array of float64
 * that the caller has zeroed (and, on several ranks, sums over the ranks before dividing).  Geometry as in
 * pmx_apply_transfer: logical shape[0..ndim) at global index start[], byte strides per field, ndim 1..3, elsize 4
 * (complex64) or 8 (complex128) per component; a and b share the shape and start.  kedges (nk + 1) and muedges
 * (nmu + 1, or NULL when nmu = 0) are DEVICE arrays of float64.
 *
 * Per stored mode, with signed index s_d (global index i_d, minus N_d when i_d >= N_d / 2), all in double:
 *   k_d = ((s_d * (2 pi / N_d)) * N_d) / L_d,   |k| = sqrt((k_0^2 + k_1^2) + k_2^2),
 *   mu = (sum_d k_d los_d) / |k| (0 at k = 0),   v = V a conj(b) / prod_d sinc(pi s_d / N_d)^deconv_pow.
 * A mode is in k bin j when kedges[j] <= |k| < kedges[j + 1] (dropped otherwise), in mu bin m when
 * muedges[m] <= mu < muedges[m + 1], the last bin closed on the right.  hermitian = 1: a mode whose index along the
 * last axis is neither 0 nor N/2 stands for itself (weight 1, value v, at mu) and its conjugate (weight 1, value
 * conj(v), at -mu); every other mode has weight 1.  L_ell are the Legendre polynomials.
 *
 * Layout of acc (S = 4 + 2 npoles doubles per k bin, then 5 per (k, mu) cell):
 *   acc[j*S + 0]            sum w                 acc[j*S + 1]            sum w |k|
 *   acc[j*S + 2]            sum w Re v            acc[j*S + 3]            sum w Im v
 *   acc[j*S + 4 + 2p]       sum w Re(v L_ell_p(mu))    acc[j*S + 5 + 2p]  sum w Im(v L_ell_p(mu))
 *   acc[nk*S + (j*nmu + m)*5 + {0, 1, 2, 3, 4}]   sum w, sum w |k|, sum w mu, sum w Re v, sum w Im v
 * Sums are added with float atomics: the last bits may differ from run to run.  nk, nmu, npoles above the
 * PMX_POWER_MAX_* limits return PMX_EUNSUPPORTED. */
int pmx_power_project(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a, const int64_t *a_strides,
                      const void *b, const int64_t *b_strides, const int64_t *shape, const int64_t *start,
                      const int64_t *nmesh, const double *boxsize, const double *kedges, const double *muedges,
                      double *acc, void *stream);

/* The adjoint of pmx_power_project with respect to the fields (pmesh_amd.power.power_spectrum_vjp): reads a (and b)
 * once and writes grad_a (and grad_b; both NULL for the auto spectrum) once, blocks of the shape and element size of a
 * with their own byte strides, not aliasing a or b.  Arguments, limits and per-mode quantities are those of
 * pmx_power_project: per stored mode m its k bin j, mu, its mu bin mubin(mu), D_m = prod_d sinc(pi s_d / N_d)^deconv_pow,
 * h_m = 1 when the mode also stands for its conjugate (hermitian = 1, last-axis index neither 0 nor N/2), else 0, and
 * w_m = 1 + h_m.
 *
 * coef is a DEVICE array of float64 that the caller builds from the cotangents v_* of the power-like columns and the
 * (global) counts; its layout is that of acc without the count, |k| and mu columns (C = 2 + 2 npoles doubles per k
 * bin, then 2 per (k, mu) cell):
 *   coef[j*C + {0, 1}]                         Re, Im of c1[j]    = v_power[j] / modes[j]
 *   coef[j*C + 2 + 2p + {0, 1}]                Re, Im of cp[p][j] = (2 ell_p + 1) v_poles[ell_p][j] / modes[j]
 *   coef[nk*C + (j*nmu + m)*2 + {0, 1}]        Re, Im of c2[j, m] = v_power2d[j, m] / modes2d[j, m]
 * each 0 where the count is 0.  With
 *   F_m(mu) = c1[j] + sum_p L_ell_p(mu) cp[p][j] + c2[j, mubin(mu)]     (the last term 0 when mu is outside muedges)
 *   q_m     = (V / D_m) (conj(F_m(mu_m)) + h_m F_m(-mu_m)),             L_ell(-mu) = (-1)^ell L_ell(mu)
 * the kernel writes, in double,
 *   grad_a = conj(q) b / w,   grad_b = q a / w        (cross)
 *   grad_a = 2 Re(q) a / w                            (auto)
 * and 0 for a mode outside kedges: for L = Re sum conj(v) P over every power-like column, Re sum_m w_m conj(u_m)
 * grad_m is the derivative of L along u.  A tile keeps a window of coefficient rows in LDS as pmx_power_project keeps
 * its window of sums; there are no atomics and the result is deterministic. */
int pmx_power_vjp(const pmx_power *p, int32_t ndim, int32_t elsize, const void *a, const int64_t *a_strides,
                  const void *b, const int64_t *b_strides, void *grad_a, const int64_t *grad_a_strides, void *grad_b,
                  const int64_t *grad_b_strides, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                  const double *boxsize, const double *kedges, const double *muedges, const double *coef,
                  void *stream);

/* ---- binned bispectrum (what bskit-style estimators compose from ComplexField.apply, c2r and products of real
 * fields: pmesh_amd.bispectrum.bispectrum) --------------------------------------------------------------------------
 * Shells are the k bins of pmx_power_project: shell(m) = j when kedges[j] <= |k_m| < kedges[j + 1], with k_d and |k|
 * computed as stated there, so a mode is in the same shell in both. */

#define PMX_BISPEC_MAX_SHELLS 64           /* shells per call */
#define PMX_BISPEC_MAX_TRIANGLES 45760     /* triples i <= j <= l of 64 shells */

/* Splits the local complex block a into nb shell spectra in one read, replacing one masked copy of the spectrum per
 * shell (ComplexField.apply with a mask on |k|): for every stored mode m and every shell s
 *   out[s][m] = a[m] / prod_d sinc(pi s_d / N_d)^deconv_pow   when shell(m) == s   (divided axis by axis, d = 0, 1, 2)
 *               0                                             otherwise,
 * and with unit != 0 the indicator: 1 in place of the (deconvolved) mode; a is then not read and may be NULL.  Every
 * element of every output is written: the outputs may be raw memory.  Geometry as in pmx_power_project: logical
 * shape[0..ndim) at global index start[], byte strides a_strides for a and out_strides (one set of ndim strides) for
 * all outputs, ndim 1..3, elsize 4 (complex64) or 8 (complex128) per component, any axis order (transposed or
 * untransposed, compressed or full spectra).  out is a host array of nb device pointers; kedges a DEVICE array of
 * nb + 1 float64.  nb above PMX_BISPEC_MAX_SHELLS returns PMX_EUNSUPPORTED. */
int pmx_bispec_shells(int32_t ndim, int32_t elsize, int32_t nb, int32_t deconv_pow, int32_t unit, const void *a,
                      const int64_t *a_strides, void *const *out, const int64_t *out_strides, const int64_t *shape,
                      const int64_t *start, const int64_t *nmesh, const double *boxsize, const double *kedges,
                      void *stream);

/* Adds, for each of ntri triples (i, j, l) = triangles[3 t .. 3 t + 3) (a DEVICE array of int32),
 *   acc[t] += sum_x fields[i][x] * fields[j][x] * fields[l][x]        ((D_i D_j) D_l, products and sums in double)
 * over the cells x of nb real blocks of one logical shape[0..ndim) and one set of byte strides (a padded last axis is
 * a stride), elsize 4 or 8, replacing one (D_i * D_j * D_l).sum() over whole fields per triple: every block is read
 * from device memory once per call, whatever ntri.  fields is a host array of nb device pointers; acc a DEVICE array
 * of ntri float64 that the caller has zeroed (and, on several ranks, sums over the ranks).  work is a DEVICE array of
 * work_doubles >= ntri float64 of any content: it holds one row of ntri partial sums per workgroup (at most 512 rows
 * are used; fewer rows, fewer workgroups), which a second kernel adds into acc in fixed order — the result is the same
 * bit for bit from run to run for the same shapes and work_doubles.  A triple that names a shell outside [0, nb) gives
 * NaN.  Consecutive triples that share (i, j) reuse the pair product.  nb above PMX_BISPEC_MAX_SHELLS or ntri above
 * PMX_BISPEC_MAX_TRIANGLES returns PMX_EUNSUPPORTED. */
int pmx_bispec_reduce(int32_t ndim, int32_t elsize, int32_t nb, const void *const *fields, const int64_t *strides,
                      const int64_t *shape, int32_t ntri, const int32_t *triangles, double *acc, double *work,
                      int64_t work_doubles, void *stream);

/* The adjoint of pmx_bispec_reduce with respect to the fields (pmesh_amd.bispectrum.bispectrum_vjp): for every shell
 * s < nb and every cell x
 *   outs[s][x] = sum over e in [offsets[s], offsets[s + 1]) of weights[e] * (fields[pairs[2 e]][x] * fields[pairs[2 e + 1]][x]),
 * products and sums in double, added in list order and rounded once to the element type: the same bits from run to
 * run.  It replaces one weighted product of two whole fields per entry: every block is read once and every output
 * written once per call, whatever npairs, with no atomics.  Blocks as in pmx_bispec_reduce: nb real blocks of one
 * logical shape[0..ndim), one set of byte strides (shared by fields and outs; a padded last axis is a stride, and the
 * padding is not touched) and elsize 4 or 8.  fields and outs are host arrays of nb device pointers; outs[s] may be
 * fields[s] (the in-place use: a cell of every field is read before that cell of any output is written), and no
 * other overlap is allowed.  offsets (nb + 1 int32, non-decreasing, offsets[nb] <= npairs), pairs (npairs x 2 int32)
 * and weights (npairs float64) are DEVICE arrays; offsets outside [0, npairs] are clamped.  A shell with an empty
 * range gets zeros: every cell of every output is written.  A pair that names a shell outside [0, nb) contributes
 * nothing.  Consecutive entries that share pairs[2 e] reuse its value.  nb above PMX_BISPEC_MAX_SHELLS or npairs
 * above 3 PMX_BISPEC_MAX_TRIANGLES returns PMX_EUNSUPPORTED. */
int pmx_bispec_pairsum(int32_t ndim, int32_t elsize, int32_t nb, const void *const *fields, void *const *outs,
                       const int64_t *strides, const int64_t *shape, int32_t npairs, const int32_t *offsets,
                       const int32_t *pairs, const double *weights, void *stream);

/* The adjoint of pmx_bispec_shells with respect to the field: for every stored mode m of the local complex block
 *   out[m] = in[shell(m)][m] / prod_d sinc(pi s_d / N_d)^deconv_pow   (divided axis by axis, d = 0, 1, 2)
 *            0                                                        when m is in no shell,
 * with |k|, shell(m) and the window computed as in pmx_bispec_shells, so a mode on an edge is in the same shell in
 * both.  Only the one spectrum a mode belongs to is read; every element of out is written (it may be raw memory) and
 * out must not be one of the inputs.  Geometry and layouts as in pmx_bispec_shells: in is a host array of nb device
 * pointers to blocks of one set of byte strides in_strides, kedges a DEVICE array of nb + 1 float64.  nb above
 * PMX_BISPEC_MAX_SHELLS returns PMX_EUNSUPPORTED. */
int pmx_bispec_shells_vjp(int32_t ndim, int32_t elsize, int32_t nb, int32_t deconv_pow, const void *const *in,
                          const int64_t *in_strides, void *out, const int64_t *out_strides, const int64_t *shape,
                          const int64_t *start, const int64_t *nmesh, const double *boxsize, const double *kedges,
                          void *stream);

/* ---- initial conditions: tabulated transfers and second-order LPT (the reference's examples/nbody.py:245-282 builds
 * its linear field with a tabulated P(k) through Field.apply; nbody/genic.py:121-166 the 2LPT displacements) --------
 * Geometry as in pmx_apply_transfer: a local block of logical shape[0..ndim) at global index start[], byte strides
 * per array, ndim 1..3, elsize 4 or 8 per (real) component.  Wavenumbers as there: k_d = w_d N_d / L_d with
 * w_d = 2 pi / N_d * (i - N_d [i >= N_d / 2]), k^2 = (k_0^2 + k_1^2) + k_2^2, all in double. */

#define PMX_KTABLE_MAX 8192            /* entries of a pmx_ktable */

typedef struct pmx_ktable {
    int32_t n;                         /* entries: 2 .. PMX_KTABLE_MAX */
    int32_t loglog;                    /* 0: x = k, y = t;  1: x = ln k, y = ln t (the caller takes the logarithms) */
    double amplitude;
    double left, right;                /* T below the first / above the last tabulated k */
    double kmin, kmax;                 /* the first and last tabulated k (not their logarithms) */
    double inv_step;                   /* > 0: x is uniform with step 1 / inv_step (the search starts from a closed-form
                                          guess; any x still gives the same result); 0: no guess */
    const double *x;                   /* device: n strictly increasing values */
    const double *y;                   /* device: n values */
} pmx_ktable;

/* out[m] = T(|k|) * in[m] over a complex block, |k| = sqrt(k^2); in may equal out.
 *   T(|k|) = amplitude * left       for |k| < kmin
 *            amplitude * right      for |k| > kmax
 *            amplitude * f(u)       otherwise, u = |k| (loglog = 0) or ln |k| (loglog = 1),
 * where g(u) = y[j] + s_j (u - x[j]) for x[j] <= u < x[j + 1], s_j = (y[j + 1] - y[j]) / (x[j + 1] - x[j]), clamped to
 * y[0] / y[n - 1] outside [x[0], x[n - 1]] (numpy.interp), and f = g (loglog = 0) or exp(g) (loglog = 1).  j is found by
 * binary search over x in device memory, from the guess (u - x[0]) inv_step when inv_step > 0.  n outside 2 .. PMX_KTABLE_MAX returns PMX_EUNSUPPORTED. */
int pmx_apply_ktable(const pmx_ktable *t, int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides,
                     void *out, const int64_t *out_strides, const int64_t *shape, const int64_t *start,
                     const int64_t *nmesh, const double *boxsize, void *stream);

/* The adjoint of pmx_apply_ktable with respect to the table values (pmesh_amd.transfer.Tabulated.apply_vjp): reads the
 * complex blocks in and v once and ADDS into grad, a device array of n float64 that the caller has zeroed (and sums
 * over the ranks),
 *   grad[i] += sum_m w_m Re(conj(v_m) in_m) e_i(|k_m|),
 * with w_m = 2 when hermitian = 1 and the mode's last-axis index is neither 0 nor N/2 (the rule of pmx_power_project),
 * else 1, and e_i the derivative of the interpolant with respect to y[i] (loglog = 0) or to ln-space y[i] times f
 * (loglog = 1), following numpy.interp's rules as stated for pmx_apply_ktable: for kmin <= |k| <= kmax and u = |k| or
 * ln |k|,
 *   u <= x[0]:      e_0 = E;   u >= x[n - 1]:  e_{n-1} = E;
 *   x[j] < u < x[j + 1] (the same search):  e_j = (1 - f) E, e_{j+1} = f E,  f = (u - x[j]) / (x[j + 1] - x[j]),
 * E = 1 (loglog = 0) or exp(g(u)) (loglog = 1), every other e_i = 0, and all e_i = 0 for |k| < kmin or |k| > kmax
 * (left and right are constants).  The caller multiplies by the amplitude and, for loglog, divides grad[i] by t[i]
 * (d ln t_i = d t_i / t_i).  A workgroup sums into an LDS copy of grad (n doubles) and adds its non-zero entries with
 * float atomics once: the last bits may differ from run to run. */
int pmx_ktable_vjp(const pmx_ktable *t, int32_t hermitian, int32_t ndim, int32_t elsize, const void *in,
                   const int64_t *in_strides, const void *v, const int64_t *v_strides, const int64_t *shape,
                   const int64_t *start, const int64_t *nmesh, const double *boxsize, double *grad, void *stream);

/* The tangent of pmx_apply_ktable along the table values (pmesh_amd.transfer.Tabulated.apply_jvp): dy is a device
 * array of n float64, the tangent of y (for loglog = 1 of ln t: dt / t).  out[m] = T'(|k|) in[m], in may equal out,
 *   T'(|k|) = amplitude * g'(u)             (loglog = 0)
 *             amplitude * exp(g(u)) g'(u)   (loglog = 1)      for kmin <= |k| <= kmax, 0 outside,
 * with g as in pmx_apply_ktable and g' the same interpolation (same j, same clamping) of dy over x. */
int pmx_apply_ktable_jvp(const pmx_ktable *t, const double *dy, int32_t ndim, int32_t elsize, const void *in,
                         const int64_t *in_strides, void *out, const int64_t *out_strides, const int64_t *shape,
                         const int64_t *start, const int64_t *nmesh, const double *boxsize, void *stream);

/* Reads the complex block `in` once and writes, for each of nout (1..3) pairs (i, j) = (pairs[2 p], pairs[2 p + 1]),
 * out[p][m] = (k_i k_j / k^2) * in[m] (0 at k = 0) with byte strides out_strides[3 p .. 3 p + 3).  pairs, out and
 * out_strides are host arrays; an out[p] may be `in` itself when it has in's strides. */
int pmx_lpt_hessian(int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides, int32_t nout,
                    const int32_t *pairs, void *const *out, const int64_t *out_strides, const int64_t *shape,
                    const int64_t *start, const int64_t *nmesh, const double *boxsize, void *stream);

/* The second-order LPT source over real blocks: in (host array of device pointers) holds ndim diagonal components
 * phi_00 .. phi_{ndim-1 ndim-1}, then the off-diagonal ones phi_01 (2-d); phi_01, phi_02, phi_12 (3-d), byte strides
 * in_strides[3 q .. 3 q + 3) each.  Writes, in double and in this order of operations,
 *   out = scale * (phi_00 phi_11 - phi_01 phi_01)                                                          (2-d)
 *   out = scale * (((((phi_00 phi_11 + phi_11 phi_22) + phi_22 phi_00) - phi_01^2) - phi_02^2) - phi_12^2)  (3-d)
 * out may equal in[0] (same strides); ndim 2 or 3. */
int pmx_lpt2_source(int32_t ndim, int32_t elsize, const void *const *in, const int64_t *in_strides, void *out,
                    const int64_t *out_strides, const int64_t *shape, double scale, void *stream);

/* ---- gradients of second-order LPT (the reference's pmesh/abopt.py chains, per component, the vjp of apply_transfer
 * with the conjugated factor and the c2r / r2c vjps: pmesh_amd.lpt.lpt_vjp / lpt_jvp) ---------------------------------
 * Geometry as above. */

/* The adjoint contraction over complex blocks, replacing abopt.py's transfer vjp (x * conj(tf(k))) summed over
 * components: out[m] = (accumulate ? out[m] : 0) + sum_c f_c(k) in[c][m] for c = 0, 1, .., nin - 1 in that order
 * (nin 1..6), in double, where for (a, b) = (factors[2 c], factors[2 c + 1])
 *   f_c = k_a k_b / k^2      (b >= 0: a Hessian factor, real)
 *   f_c = -i k_a / k^2       (b < 0: the conjugate of the gradient factor i k_a / k^2 of Transfer.dx1)
 * and every f_c is 0 at k = 0.  in (host array of device pointers), in_strides (3 per input) and factors are host
 * arrays; out may equal in[0] (same strides). */
int pmx_lpt_contract(int32_t ndim, int32_t elsize, int32_t nin, const void *const *in, const int64_t *in_strides,
                     const int32_t *factors, int32_t accumulate, void *out, const int64_t *out_strides,
                     const int64_t *shape, const int64_t *start, const int64_t *nmesh, const double *boxsize,
                     void *stream);

/* The vjp of pmx_lpt2_source with respect to its inputs, replacing abopt.py's products of the cotangent with the
 * partial derivatives of the source: with a = scale * g[m] (g a real block) and phi the 3 (2-d) or 6 (3-d) components
 * in[] in the order of pmx_lpt2_source, writes in double
 *   2-d: out[0] = a phi_11, out[1] = a phi_00, out[2] = a (-2 phi_01)
 *   3-d: out[0] = a (phi_11 + phi_22), out[1] = a (phi_22 + phi_00), out[2] = a (phi_00 + phi_11),
 *        out[3] = a (-2 phi_01), out[4] = a (-2 phi_02), out[5] = a (-2 phi_12).
 * Every input of an element is read before any output of it is written: out[p] may equal in[p] (same strides). */
int pmx_lpt2_source_vjp(int32_t ndim, int32_t elsize, const void *g, const int64_t *g_strides, const void *const *in,
                        const int64_t *in_strides, void *const *out, const int64_t *out_strides, const int64_t *shape,
                        double scale, void *stream);

/* The jvp of pmx_lpt2_source, replacing abopt.py's product rule over real fields: with phi = in[] and phi' = tangent[]
 * (the same order of components), writes in double and in this order of operations
 *   out = scale * ((phi_00 phi'_11 + phi'_00 phi_11) - 2 (phi_01 phi'_01))                                  (2-d)
 *   s = (phi_00 phi'_11 + phi'_00 phi_11) + (phi_11 phi'_22 + phi'_11 phi_22);  s = s + (phi_22 phi'_00 + phi'_22 phi_00);
 *   s = s - 2 (phi_01 phi'_01);  s = s - 2 (phi_02 phi'_02);  s = s - 2 (phi_12 phi'_12);  out = scale * s     (3-d)
 * out may equal tangent[0] (same strides); ndim 2 or 3. */
int pmx_lpt2_source_jvp(int32_t ndim, int32_t elsize, const void *const *in, const int64_t *in_strides,
                        const void *const *tangent, const int64_t *tangent_strides, void *out,
                        const int64_t *out_strides, const int64_t *shape, double scale, void *stream);

/* ---- survey power multipoles with a local line of sight (the FFT form of the Yamamoto estimator: Bianchi et al. 2015,
 * Scoccimarro 2015, Hand et al. 2017; what nbodykit's ConvolvedFFTPower computes; pmesh_amd.survey) -------------------
 * Geometry as in pmx_apply_transfer, 3-d blocks only.  Definitions:
 *   Cell position.  Cell g (global index, 0 <= g_d < N_d) sits at x_d = (g_d * L_d) / N_d, in double and in this order
 *     of operations: the position paint assigns to that cell, not wrapped to negative values.
 *   Direction.  origin is the observer, in the box coordinates of particle positions; r = x - origin is never wrapped
 *     periodically; r_hat = r / |r|.
 *   Real orthonormal harmonics Y_lm without the Condon-Shortley phase.  With
 *     N_lm = sqrt((2l+1) / (4 pi) (l-|m|)! / (l+|m|)!) and P_l^m(c) = (1 - c^2)^(m/2) d^m P_l / dc^m,
 *       m = 0:  N_l0 P_l(cos th)
 *       m > 0:  sqrt2 N_lm P_l^m(cos th) cos(m ph)
 *       m < 0:  sqrt2 N_l|m| P_l^|m|(cos th) sin(|m| ph)
 *     for a unit vector (x, y, z) with cos th = z, ph = atan2(y, x): Y_22 is proportional to +(x^2 - y^2), Y_21 to +xz,
 *     Y_2,-1 to +yz.  For a zero vector (r = 0 or k = 0), Y_00 = 1 / sqrt(4 pi) and every Y_lm with l > 0 is 0.
 *   The multipole field.  With r2c in the package's convention (divided by prod N, phase exp(-i k.x)),
 *       A_l(k) = (4 pi / (2l+1)) sum_m Y_lm(k_hat) * r2c[F * Y_lm(r_hat)](k)
 *     which by the addition theorem is (1 / prod N) sum_x F(x) L_l(k_hat . r_hat) exp(-i k.x), L_l the Legendre
 *     polynomial, taken as [l == 0] at k = 0 or r = 0; A_0 = r2c[F].
 *   The result.  P_l(bin) = (2l+1) V <A_0 conj(A_l)> with the bins, counts, Hermitian weighting and rank sum of
 *     pmx_power_project.  Even orders only: for odd l, A_l is anti-Hermitian and the mirrored-mode rule does not hold.
 * Both entries evaluate Y_lm as a Cartesian polynomial of the unit vector (no trigonometric calls, one sqrt and one
 * division per element), compute in double and round once on the store, take any axis order (C, transposed, padded,
 * strided) and elsize 4 or 8 per (real) component, and return PMX_EUNSUPPORTED for ndim != 3, ell not in {0, 2, 4} or
 * |m| > ell. */

/* Real blocks: out = in * Y_lm(r_hat) with r_hat the direction from origin[0..3) to the cell.  out may alias in (same
 * strides); every element of out is written, so out may be raw memory. */
int pmx_ylm_weight(int32_t ell, int32_t m, int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides,
                   void *out, const int64_t *out_strides, const int64_t *shape, const int64_t *start,
                   const int64_t *nmesh, const double *boxsize, const double *origin, void *stream);

/* Complex blocks: acc = beta * acc + (4 pi / (2l+1)) Y_lm(k_hat) * in, beta 0 or 1; with beta = 0 acc is not read and
 * may be raw memory.  k as in pmx_apply_transfer; only its direction matters. */
int pmx_ylm_accumulate(int32_t ell, int32_t m, int32_t beta, int32_t ndim, int32_t elsize, const void *in,
                       const int64_t *in_strides, void *acc, const int64_t *acc_strides, const int64_t *shape,
                       const int64_t *start, const int64_t *nmesh, const double *boxsize, void *stream);

/* ---- interlaced painting: the combine pass (Hockney & Eastwood; Sefusatti et al. 2016; what nbodykit's
 * interlaced=True computes; pmesh_amd.interlace) ----------------------------------------------------------------------
 * For every mode of a strided block of a spectrum (global index g_d = idx_d + start_d, ndim 1 to 3):
 *     acc = (a * acc + b * exp(i * theta) * in) / prod_d sinc(w_d / 2)^deconv_pow,    theta = sum_d shift_d * w_d
 * with the circular frequency w_d = 2 pi / N_d * (g_d - N_d [g_d >= N_d / 2]) (the Nyquist frequency negative, pmesh's
 * convention and the one nbodykit's interlacing uses) and `shift` in cells, any real numbers: exp(i theta) undoes the
 * displacement of a mesh painted with the transform shifted by `shift`.  deconv_pow >= 0, 0: no division.  With a == 0
 * acc is not read and may be raw memory.  elsize 4 or 8 per (real) component of complex f4 / f8 storage; the
 * arithmetic is in double, rounded once on the store.  The phase is formed from the signed mode numbers,
 * theta / pi = sum_d 2 shift_d m_d / N_d reduced term by term, so it is as accurate at |m| = 2^16 as at m = 1.  `in`
 * and `acc` take any axis order (C, transposed, padded, strided), each its own; the byte ranges they reach must not
 * overlap (PMX_EINVAL).  PMX_EUNSUPPORTED for a plane of 2^31 modes or more. */
int pmx_phase_combine(int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides, void *acc,
                      const int64_t *acc_strides, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                      const double *shift, double a, double b, int32_t deconv_pow, void *stream);

/* ---- binned correlation function (what nbodykit's FFTCorr computes: a conj(b) transformed back and binned by
 * RealField.x; pmesh_amd.correlation) -----------------------------------------------------------------------------------
 * Definition, for a 1-, 2- or 3-d real mesh (f4 or f8) with the spectra a and b (b = a: the auto correlation):
 *   1. S = a conj(b) / prod_d sinc(w_d / 2)^deconv_pow                                  (pmx_spectral_product)
 *   2. xi = c2r(S): with pmesh's normalisation xi(x) is the mean over y of A(y + x) B(y).  The k = 0 mode is kept;
 *      removing the mean is the caller's business.
 *   3. per cell, in double: r_d = (s_d * L_d) / N_d with the signed index s_d (global index i_d, minus N_d when
 *      i_d >= N_d / 2) — what RealField.x of an f8 mesh holds, with the same two roundings —
 *      |r| = sqrt((r_0^2 + r_1^2) + r_2^2),   mu = ((r_0 los_0 + r_1 los_1) + r_2 los_2) / |r| (0 at r = 0).
 *   4. a cell is in r bin j when redges[j] <= |r| < redges[j + 1] (dropped otherwise), in mu bin m when
 *      muedges[m] <= mu < muedges[m + 1], the last bin closed on the right.  Every cell has weight 1: there is no
 *      Hermitian doubling on the real side.
 *   5. the raw sums below are added over the ranks first, then divided: xi_l(r) = (2l + 1) sum x L_l(mu) / count.
 *
 * pmx_corr_project adds the sums of the local real block x (steps 3 to 5; any real mesh, not only a xi) into `acc`, a
 * zeroed DEVICE array of float64.  p: nk is the number of r bins, nmu, npoles, poles, los as in pmx_power_project,
 * volume multiplies every value, hermitian and deconv_pow must be 0 (PMX_EINVAL); the PMX_POWER_MAX_* limits apply
 * (PMX_EUNSUPPORTED).  elsize 4 or 8: one real element, loaded as such and widened to double.  Any byte strides: C
 * order, the padded last axis of an in-place transform, transposed views, a block at `start` inside a larger mesh.
 * redges (nk + 1) and muedges (nmu + 1, or NULL) are DEVICE arrays of float64.
 * Layout of acc (S = 3 + npoles doubles per r bin, then 4 per (r, mu) cell):
 *   acc[j*S + 0] count    acc[j*S + 1] sum |r|    acc[j*S + 2] sum x    acc[j*S + 3 + p] sum x L_ell_p(mu)
 *   acc[nk*S + (j*nmu + m)*4 + {0, 1, 2, 3}]   count, sum |r|, sum mu, sum x
 * One read of the block, nothing mesh-sized written: one workgroup per 16 x 16 x 64 tile in memory order keeps the
 * window of r bins its index box can reach in LDS (|r| is monotone in each |r_d|; a tile may straddle N / 2), sums
 * runs of cells of one bin in registers, and adds the window to acc once per tile and touched bin (float atomics: the
 * last bits may differ from run to run). */
int pmx_corr_project(const pmx_power *p, int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides,
                     const int64_t *shape, const int64_t *start, const int64_t *nmesh, const double *boxsize,
                     const double *redges, const double *muedges, double *acc, void *stream);

/* The adjoint of pmx_corr_project with respect to the mesh: writes every cell of the real block g (its own byte
 * strides; raw memory is allowed) with
 *   volume * (c1[j] + sum_p cp[p][j] L_ell_p(mu) + c2[j, mubin(mu)])      (the last term 0 when mu is outside muedges)
 * for the cell's r bin j, and 0 for a cell outside redges.  coef is a DEVICE array of float64 in the layout of acc
 * without the count, |r| and mu columns (C = 1 + npoles doubles per r bin, then 1 per (r, mu) cell):
 *   coef[j*C + 0] c1[j]     coef[j*C + 1 + p] cp[p][j]     coef[nk*C + j*nmu + m] c2[j, m]
 * The tiles, windows and bin search are those of pmx_corr_project, so every cell reads the bin the forward put it in.
 * No atomics; the result is deterministic. */
int pmx_corr_vjp(const pmx_power *p, int32_t ndim, int32_t elsize, void *g, const int64_t *g_strides,
                 const int64_t *shape, const int64_t *start, const int64_t *nmesh, const double *boxsize,
                 const double *redges, const double *muedges, const double *coef, void *stream);

/* out = [out +] scale * x * (conj_y ? conj(y) : y) / prod_d sinc(w_d / 2)^deconv_pow over a strided block of a
 * spectrum (w_d as in pmx_phase_combine; ndim 1 to 3; elsize 4 or 8 per component; the arithmetic in double, rounded
 * once on the store): the product of step 1 above and both products of its gradient, one streaming kernel with two
 * reads and one write per mode (three reads when accumulating).  x, y and out take any axis order, each its own
 * strides; out may be exactly x or exactly y (same pointer and strides), and x may be y; any other overlap of out with
 * an input is refused (PMX_EINVAL).  Without `accumulate` out is not read and may be raw memory.  PMX_EUNSUPPORTED for
 * a plane of 2^31 modes or more. */
int pmx_spectral_product(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides, const void *y,
                         const int64_t *y_strides, void *out, const int64_t *out_strides, const int64_t *shape,
                         const int64_t *start, const int64_t *nmesh, double scale, int32_t conj_y, int32_t accumulate,
                         int32_t deconv_pow, void *stream);

/* ---- Poisson-sampled particles from a real mesh (what nbodykit's LogNormalCatalog does on the host: Poisson counts of
 * the cells, the cell coordinates repeated, uniform offsets; pmesh_amd.mock) ---------------------------------------------
 * The sampling rule.  Every random number is one call of Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53,
 * 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85) with
 *     key = (seed & 0xffffffff, seed >> 32),     counter = (g & 0xffffffff, g >> 32, j, stream)
 * where g is the GLOBAL C-order index of the cell over nmesh, (i_0 N_1 + i_1) N_2 + i_2 (likewise in 1-d and 2-d): a
 * cell's draws depend on no block, rank or launch shape.  Its words are w_0 .. w_3.
 *   rate     in double whatever the field's element type: lam = scale * x (PMX_POISSON_LINEAR) or
 *            lam = scale * exp(bias * x) (PMX_POISSON_EXP).  A cell whose lam is NaN, negative, infinite or above
 *            PMX_POISSON_MAX_RATE gets the count 0 and adds 1 to `flagged`.
 *   count    (stream 0) n = max(1, ceil(lam / PMX_POISSON_CHUNK_RATE)) chunks of rate lam_j = lam / n; chunk j takes one
 *            call with counter word j, u = ((w_0 >> 5) * 2^26 + (w_1 >> 6) + 1) * 2^-53 in (0, 1], and is drawn by
 *            inversion: k = 0; p = exp(-lam_j); s = p; while (u > s && k < PMX_POISSON_MAX_STEPS) { k += 1;
 *            p = p * lam_j / k; s += p; } (the multiplication and the division each round once).  The count of the
 *            cell is the sum of its chunks' k, a uint32.
 *   position (stream 1) particle p of the cell takes one call with j = p; u_d = (w_d + 0.5) * 2^-32 for d < ndim and
 *            x_d = ((i_d - 0.5) + u_d) * (L_d / N_d), plus L_d where that is negative (and 0 should that sum round to
 *            L_d): uniform in the cell centred on the grid point i_d L_d / N_d, the convention of the windows here — a
 *            nearest-grid-point paint of the particles returns the counts.
 *   order    cells in the C order of the local block, the particles of a cell in the order of p.
 * The local cells, in C order, are cut into segments of PMX_POISSON_SEGMENT cells — a constant of the ABI, not a launch
 * parameter — and the four entries are called in this order, on one stream: */
#define PMX_POISSON_SEGMENT 4096         /* cells per segment */
#define PMX_POISSON_MAX_RATE (1 << 20)   /* the largest rate of a cell */
#define PMX_POISSON_CHUNK_RATE 16        /* a cell's rate is drawn in chunks of at most this rate */
#define PMX_POISSON_MAX_STEPS 128        /* the cap on the search steps of one chunk (P(k > 128 | 16) < 1e-60) */
#define PMX_POISSON_LINEAR 0             /* mode: lam = scale * x */
#define PMX_POISSON_EXP 1                /* mode: lam = scale * exp(bias * x) */

/* *total += the sum of the rates (mode, scale, bias as above; refused rates included as they are) of the real block x:
 * a DEVICE double, one float atomic per segment (the last bits may differ from run to run).  elsize 4 or 8: one real
 * element, loaded as such and widened to double; any byte strides (C order, a padded last axis, transposed or strided
 * views).  ndim 1 to 3.  The mean of exp(bias x) of a lognormal mock and the expected number of particles. */
int pmx_poisson_rate_sum(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides, const int64_t *shape,
                         int32_t mode, double scale, double bias, double *total, void *stream);

/* The counts of the block x (read as in pmx_poisson_rate_sum) at `start` inside the mesh `nmesh`, one lane per cell:
 *   counts     uint32 per local cell, contiguous in the C order of the block            (DEVICE, prod(shape) entries)
 *   seg_sums   the sum of the counts of every segment, reduced in LDS   (DEVICE int64, ceil(prod(shape) / SEGMENT))
 *   flagged    += the number of cells whose rate is refused; the caller zeroes it               (DEVICE int64)
 * Integer results: deterministic.  Moves elsize + 4 bytes per cell.  PMX_EINVAL for a block that does not lie inside the
 * mesh, PMX_EUNSUPPORTED for an axis of 2^31 - 4096 cells or more or 2^31 segments. */
int pmx_poisson_count(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides, const int64_t *shape,
                      const int64_t *start, const int64_t *nmesh, int32_t mode, double scale, double bias,
                      uint64_t seed, uint32_t *counts, int64_t *seg_sums, int64_t *flagged, void *stream);

/* The exclusive scan of the nseg segment sums, in place: seg_sums[s] becomes the row of the first particle of segment
 * s, and *total (DEVICE int64) the number of particles.  One workgroup walks the array; no workgroup of this feature
 * waits on memory written by another.  The host reads *total (and flagged) here to allocate `pos`: the one
 * synchronisation of the sequence. */
int pmx_poisson_scan(int64_t *seg_sums, int64_t nseg, int64_t *total, void *stream);

/* The particles.  pos is a C-contiguous DEVICE array of float64, (npart, ndim), npart the *total of the scan; cell, when
 * not NULL, a DEVICE int64 array of npart entries that receives the global cell index g of every particle.  counts and
 * seg_offsets are what pmx_poisson_count and pmx_poisson_scan left.  One workgroup per segment scans the segment's
 * counts in LDS (16 KB) and walks its particles ONE LANE PER PARTICLE: the lane finds its cell by binary search in the
 * LDS offsets, so consecutive lanes write consecutive rows and a cell of thousands of particles is shared by the whole
 * workgroup.  Row offsets are 64-bit; a single segment may hold up to 2^32 - 1 particles.  Moves 4 bytes per cell and
 * 8 ndim (+ 8 with cell) bytes per particle.  Deterministic. */
int pmx_poisson_emit(int32_t ndim, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                     const double *boxsize, uint64_t seed, const uint32_t *counts, const int64_t *seg_offsets,
                     int64_t npart, double *pos, int64_t *cell, void *stream);

/* ---- friends-of-friends groups of particles (what nbodykit's FOF does on the host with a kd-tree; pmesh_amd.fof) -------
 * The rule.  Positions are (n, ndim) rows, ndim 1 to 3, float or double (a float is widened exactly); all arithmetic is
 * in double, every operation rounding once.
 *   wrap     w_d = x_d - L_d * floor(x_d / L_d), then w_d + L_d where that is negative and 0 where it is >= L_d: rows
 *            lie in [0, L_d).  A row with a coordinate that is not finite adds 1 to `flagged`.
 *   friends  two rows are friends when sum_d dx_d^2 <= b^2, dx_d = w_d - w'_d; dx_d -= L_d * rint(dx_d / L_d) (the
 *            minimum image), the sum accumulated in the order d = 0, 1, 2.  b, the linking length, is finite, positive
 *            and 2 b <= min_d L_d.
 *   groups   a group is a connected component of the friendship graph over the rows of all ranks; the canonical label of
 *            a row is minid, the smallest GLOBAL row index of its group (local index plus the rows of the lower ranks).
 *            It depends on no decomposition, launch shape or order in which lanes run.
 * The passes, on the n rows a rank holds (its own and the ghosts within b of its block), all on one stream:
 *   pmx_fof_cells      wrapped rows, the cell of every row on a grid of cells of side >= b, the rows per cell
 *   (the caller)       cell_start = the exclusive scan of the counts, ncells + 1 entries
 *   pmx_fof_fill       the rows in cell order: order[slot] and the wrapped rows sorted
 *   pmx_fof_link       one lane per row: the friends of lower index in the 3^ndim neighbouring cells, hooked into a
 *                      lock-free union-find that keeps parent[x] <= x
 *   pmx_fof_flatten    parent[i] = the root of row i: the smallest local index of its component
 *   pmx_fof_minlabel   the minimum of an int64 value over every local component, written to all its members
 *   pmx_fof_group_sums per-label sums of mass, mass x wrapped displacement and mass x velocity (the halo catalogue)
 * The grid.  Axis d has ncell[d] cells of side extent_d / ncell[d] >= b starting at origin[d]; the cell of a row is
 * c_d = (int)(r_d * inv_side[d]) clamped to ncell[d] - 1, r_d = w_d - origin[d], plus L_d where that is negative.  A
 * periodic axis (bit d of `periodic`, PMX_FOF_PERIODIC_X << d) has origin 0 and covers the box: neighbours wrap, and
 * with 1 or 2 cells every cell is visited once.  An open axis covers extent_d = ncell[d] / inv_side[d] < L_d; nothing
 * wraps, and a row beyond the extent (rounding) goes to the nearer end cell.  The flat cell index is C order.
 * n <= PMX_FOF_MAX_ROWS and prod(ncell) <= PMX_FOF_MAX_ROWS: parents, slots and cells are 32-bit. */
#define PMX_FOF_MAX_ROWS 2147483647      /* rows (own and ghosts) of one rank, and cells of its grid */
#define PMX_FOF_CELLS_PER_ROW 2          /* the grid a caller lays has at most this many cells per row (and one) */
#define PMX_FOF_PERIODIC_X 1             /* `periodic`: axis 0 wraps; axis d: PMX_FOF_PERIODIC_X << d */

/* wpos[i, d] = the wrapped row i (DEVICE double, (n, ndim) contiguous), cell_of[i] its flat cell (DEVICE int32),
 * counts[c] += 1 per row of cell c (DEVICE int32, prod(ncell) entries, zeroed by the caller), *flagged += the rows
 * with a coordinate that is not finite (DEVICE int64; such a row lands in some valid cell).  pos: n rows of ndim
 * columns, any strides.  Moves ndim * elsize + 8 ndim + 4 bytes per row and one atomic. */
int pmx_fof_cells(int32_t ndim, const pmx_vec *pos, int64_t n, const double *boxsize, const double *origin,
                  const double *inv_side, const int64_t *ncell, int32_t periodic, double *wpos, int32_t *cell_of,
                  int32_t *counts, int64_t *flagged, void *stream);

/* order[slot] = i and spos[slot, :] = wpos[i, :] with slot = cell_start[cell_of[i]] + (cursor[cell_of[i]]++): the rows
 * in cell order.  cursor: DEVICE int32, ncells entries, zeroed by the caller.  The order of the rows INSIDE a cell
 * depends on the atomics; nothing the later passes leave depends on it. */
int pmx_fof_fill(int32_t ndim, int64_t n, const double *wpos, const int32_t *cell_of, const int32_t *cell_start,
                 int32_t *cursor, int32_t *order, double *spos, void *stream);

/* parent[i] = i for every row, then one lane per slot k (row i = order[k]): every row j < i of the 3^ndim neighbouring
 * cells that is a friend of i is united with it: find both roots; atomic-min the smaller root into the larger root's
 * slot; if the value returned was not that root, go on with the value returned.  Every loop walks strictly decreasing
 * indices; no lane waits for another.  b2 = b * b.  Afterwards two rows are in one component exactly if their parent
 * chains end at the same root. */
int pmx_fof_link(int32_t ndim, int64_t n, const double *spos, const int32_t *order, const int32_t *cell_of,
                 const int32_t *cell_start, const int64_t *ncell, int32_t periodic, const double *boxsize, double b2,
                 int32_t *parent, void *stream);

/* parent[i] = the root of row i (the smallest local index of its component), in place, a launch of its own */
int pmx_fof_flatten(int64_t n, int32_t *parent, void *stream);

/* val[i] = min over the rows j with root[j] == root[i] of val[j] (DEVICE int64, in place); *changed += the number of
 * rows whose value changed (DEVICE int64).  work: DEVICE int64 scratch of n entries.  root: what pmx_fof_flatten
 * left.  One copy, one atomic minimum per row that is not a root, one gather. */
int pmx_fof_minlabel(int64_t n, const int32_t *root, int64_t *val, int64_t *work, int64_t *changed, void *stream);

/* out[l, :] += over the rows i with l = labels[i] in 1 .. ngroups of (m_i, m_i * dx_i[0 .. ndim), m_i * v_i[0 .. ndim)):
 * out is a DEVICE double array (ngroups + 1, 1 + 2 ndim), zeroed by the caller; dx_i the minimum image of
 * wrap(pos_i) - wrap(ref[l, :]), ref a DEVICE double array (ngroups + 1, ndim) contiguous: the position of the
 * reference member of every group.  mass (one column; NULL: 1) and vel (ndim columns; NULL: 0) are optional.  Equal
 * labels are reduced within a wave before one atomic per wave, label and column: the members of a large halo do not
 * meet on one line.  The last bits depend on the order of the atomics. */
int pmx_fof_group_sums(int32_t ndim, int64_t n, const pmx_vec *pos, const int64_t *labels, const pmx_vec *mass,
                       const pmx_vec *vel, const double *ref, int64_t ngroups, const double *boxsize, double *out,
                       void *stream);

/* ---- binned pair counts of particles (what nbodykit's SimulationBoxPairCount does on the host with Corrfunc;
 * pmesh_amd.paircount) ------------------------------------------------------------------------------------------------
 * The rule.
 *   rows     pos1 and pos2 are (n, ndim) rows, ndim 1 to 3, float or double (a float is widened exactly); all arithmetic
 *            is in double, every operation rounding once.  Rows are wrapped as above; dx_d is the minimum image of the
 *            difference of the wrapped rows as above; r2 = sum_d dx_d^2 accumulated in the order d = 0, 1, 2.
 *   modes    PMX_PAIRS_1D bins by r, PMX_PAIRS_2D by (r, mu), PMX_PAIRS_PROJECTED by (rp, pi); the last two need
 *            ndim == 3 and a line-of-sight axis los in {0, 1, 2}.
 *   edges    e2[k] = edges[k] * edges[k] is formed by the caller, edges increasing and finite, edges[0] >= 0.  A pair is
 *            in r-bin k when e2[k] <= q < e2[k + 1]; q = r2 in the modes 1D and 2D, q = rp2 in the projected mode: the
 *            sum of the two dx_d^2 with d != los in ascending d.  Pairs outside [e2[0], e2[nr]) are not counted.  No
 *            square root is taken to choose a bin.
 *   mu       (2D) sub[k] = m2[k] = muedges[k]^2, muedges increasing from 0 to 1.  With z2 = dx_los^2 the mu-bin is the
 *            number of k in 1 .. nsub - 1 with z2 >= m2[k] * r2: no division; mu = 1 lands in the last bin.  A pair with
 *            r2 == 0 goes to mu-bin 0.
 *   pi       (projected) sub[k] = piedges[k], increasing from 0.  With a = |dx_los| the pi-bin is the number of k in
 *            1 .. nsub - 1 with a >= piedges[k]; pairs with a >= piedges[nsub] are not counted.
 *   pairs    every (slot of the primaries, slot of the secondaries), coincident rows included.  The entry knows no row
 *            identity: a caller that passes one set as both subtracts its self pairs, which have r2 == 0 exactly and sit
 *            in bin (0, 0) when edges[0] == 0 and nowhere otherwise.
 *   sums     per bin: npairs (int64, exact); wnpairs = sum w1_i w2_j (double); rsum = sum w1_i w2_j sqrt(q) (double).
 *            The order of the double sums is unspecified: their last bits may differ from run to run; npairs never does.
 * The bin of a pair is r-bin * nsub + sub-bin (nsub = 1 in the mode 1D); nr * nsub <= PMX_PAIRS_MAX_BINS.
 *
 * The modes with the line of sight of the pair itself (what nbodykit's SurveyDataPairCount does on the host with
 * Corrfunc's DDsmu_mocks / DDrppi_mocks; pmesh_amd.surveypairs).  Rows, edges, pairs and sums are as above; the new
 * parts:
 *   observer  the entry knows one observer, the centre of the box: o_d = L_d / 2.  For a pair of wrapped rows w_i, w_j:
 *             dx_d as above; l_d = (w_i,d + w_j,d) - L_d, two roundings: twice the offset of the pair's midpoint from the
 *             observer, of which only the direction matters.  p = dx_0 l_0 + dx_1 l_1 + dx_2 l_2, l2 = l_0^2 + l_1^2 +
 *             l_2^2, r2 = dx_0^2 + dx_1^2 + dx_2^2, each sum taken in that order; p2 = p * p.
 *   PMX_PAIRS_2D_MIDPOINT, bins of (s, mu): the r-bin comes from q = r2 as in the mode 2D.  t = r2 * l2; the mu-bin is
 *             the number of k in 1 .. nsub - 1 with p2 >= sub[k] * t, sub[k] = muedges[k]^2: no division.  A pair with
 *             t == 0 goes to mu-bin 0: r2 == 0, and a pair symmetric about the observer.  Corrfunc's DDsmu_mocks:
 *             mu^2 = (s.l)^2 / (s^2 l^2), l = (x1 + x2) / 2.
 *   PMX_PAIRS_PROJECTED_MIDPOINT, bins of (rp, pi): pi2 = p2 / l2, or 0 where l2 == 0; rp2 = r2 - pi2, or 0 where that
 *             is negative.  The r-bin comes from q = rp2 against e2.  sub[k] = piedges[k]^2 (squared by the caller,
 *             unlike PMX_PAIRS_PROJECTED, which takes piedges themselves); the pi-bin is the number of k in
 *             1 .. nsub - 1 with pi2 >= sub[k]; a pair with pi2 >= sub[nsub] is not counted.  rsum adds w sqrt(rp2).
 *             Corrfunc's DDrppi_mocks: pi = |s.l| / |l|, rp^2 = s^2 - pi^2.
 *   both      los is ignored; ndim == 3; both are symmetric under exchanging the two rows, so one set passed as both
 *             still counts every unordered pair twice.  The grid, the wrapping and the minimum image stay periodic: a
 *             caller with a survey keeps every row in [b / 2, L_d - b / 2), b the search radius (edges[nr]; in the
 *             projected mode hypot(edges[nr], piedges[nsub]): the walk over the cells must cover the bounding sphere of
 *             the cylinder), so that no two rows are closer than b through the boundary and no counted pair is a
 *             wrapped one.
 *
 * The modes with one histogram per primary row (radial profiles, enclosed and spherical-overdensity masses, counts in
 * spheres and Sigma(R) about centres; pmesh_amd.profiles).  PMX_PAIRS_1D_ROWS is PMX_PAIRS_1D and
 * PMX_PAIRS_PROJECTED_ROWS is PMX_PAIRS_PROJECTED with the sums of every primary kept apart:
 *   shared    rows, wrapping, minimum image, r2, q, the squared edges, the r-bin, the pi-bin and the pimax cut are
 *             exactly those of PMX_PAIRS_1D and PMX_PAIRS_PROJECTED: all arithmetic in double, every operation rounded
 *             once, no contraction, no square root choosing a bin.  PMX_PAIRS_PROJECTED_ROWS needs ndim == 3 and los in
 *             {0, 1, 2}; PMX_PAIRS_1D_ROWS takes ndim 1 to 3 and nsub == 1.
 *   bin       the bin of a pair (primary row i, secondary slot s) is (i * nr + rbin) * nsub + subbin, i the ROW of the
 *             primary (order1[slot]), not its slot.
 *   arrays    npairs, wnpairs and rsum are DEVICE arrays of n1 * nr * nsub entries in the caller's row order.  They are
 *             added to, as in the base modes: the caller zeroes them, and a second call with other secondaries keeps
 *             adding.
 *   limit     nr * nsub <= PMX_PAIRS_ROWS_MAX_BINS, else PMX_EINVAL.
 *   exact     npairs is exact and depends on no decomposition or launch.  The order of the double sums is unspecified,
 *             as in the base modes.  With both weights NULL, wnpairs += (double)(the count).
 *   identity  there is none: a centre that coincides with a source has r2 == 0 and is counted in bin 0 when
 *             edges[0] == 0 and nowhere otherwise.
 *   windows   above 2^23 secondaries the entry still launches once per window of 2^23 slots.  One wave per primary
 *             slot keeps the row's histogram in LDS (pmx_pairs_rows.hip) and owns the row's bins for the launch: it adds
 *             them with plain loads and stores, no global atomic.
 *
 * The modes with pairwise velocity statistics (the mean pairwise velocity v12(r), the pairwise dispersions, the
 * line-of-sight pairwise velocity in bins of (rp, pi), the pairwise estimator of Ferreira et al. 1999 for one
 * line-of-sight scalar per row; pmesh_amd.pairvel).  PMX_PAIRS_1D_VELOCITY shares everything below with PMX_PAIRS_1D,
 * PMX_PAIRS_PROJECTED_VELOCITY with PMX_PAIRS_PROJECTED, PMX_PAIRS_1D_LOS with PMX_PAIRS_1D:
 *   shared    rows, wrapping, the minimum image dx_d (primary minus secondary), r2, q, the squared edges, the r-bin, the
 *             pi-bin and the pimax cut; all arithmetic in double; every operation rounded once, no contraction; no
 *             square root chooses a bin.  npairs equals npairs of the corresponding base mode on the same arguments, to
 *             the last count.
 *   columns   weight1 and weight2 are both required.  PMX_PAIRS_1D_VELOCITY and PMX_PAIRS_PROJECTED_VELOCITY: pmx_vecs
 *             of 1 + ndim columns, (w, v_0 .. v_{ndim-1}).  PMX_PAIRS_1D_LOS: 2 columns, (w, s).  Float or double, in
 *             ROW order, read through order1 / order2 like the weights of the base modes.  A wrong ncol is PMX_EINVAL.
 *   outputs   npairs and wnpairs have nr * nsub entries, as in the base modes.  rsum has 4 * nr * nsub entries:
 *             rsum[m * nbins + b]; m = 0: sum w sqrt(q), as in the base modes; m = 1, 2, 3: the sums S1, S2, S3 below.
 *             All are added to, never overwritten.  The order of the double sums is unspecified; npairs is exact.
 *   per counted pair, with w = w1_i * w2_j:
 *   PMX_PAIRS_1D_VELOCITY, ndim 1 to 3, nsub == 1: dv_d = v_i,d - v_j,d; h = dx_0 dv_0 + dx_1 dv_1 + dx_2 dv_2 and
 *             dv2 = dv_0^2 + dv_1^2 + dv_2^2, each summed in that order over d < ndim; r = sqrt(r2); u = h / r where
 *             r2 > 0, else 0.  S1 += (w u), S2 += (w u) u, S3 += w dv2.  u is the radial pairwise velocity: negative
 *             means the pair approaches.
 *   PMX_PAIRS_PROJECTED_VELOCITY, ndim 3, los in {0, 1, 2}, sub = piedges: u = dx_los < 0 ? -dv_los : dv_los; S1, S2,
 *             S3 as above, with dv2 over all three axes.  The m = 0 sum adds w sqrt(rp2), as PMX_PAIRS_PROJECTED does.
 *   PMX_PAIRS_1D_LOS, ndim 3, nsub == 1; los is ignored.  The observer is at o_d = 0.5 * L_d, as in the midpoint
 *             modes, and the caller keeps rows in [b / 2, L_d - b / 2) as for them.  a_d = w_i,d - o_d and b_d = w_j,d -
 *             o_d, w_i and w_j the wrapped rows; a2, b2, pa = dx.a and pb = dx.b are each summed over d = 0, 1, 2 in
 *             order; ta = a2 > 0 ? pa / sqrt(a2) : 0, tb likewise; c = r2 > 0 ? 0.5 * ((ta + tb) / r) : 0; ds = s_i -
 *             s_j.  S1 += (w c) ds, S2 += (w c) c, S3 += (w ds) ds.  (Ferreira et al. 1999: v12 = S1 / S2.)
 *   self      a self pair (one set passed as both) has r2 == 0, dv == 0 and ds == 0: it adds nothing to S1 .. S3; the
 *             caller subtracts it from npairs[0] and wnpairs[0] as in the base modes.  Each statistic is even under
 *             exchanging the two rows, so one set passed as both counts every unordered pair twice, in the numerator
 *             and in the denominator alike.
 *   limit     nr * nsub <= PMX_PAIRS_VELOCITY_MAX_BINS, else PMX_EINVAL: the histogram of a workgroup holds a 32-bit
 *             count and five doubles per bin in LDS (pmx_pairs_vel.hip).
 *
 * The modes by row labels (the one-halo / two-halo split of the pairs, halotools' tpcf_one_two_halo_decomp, and the sums
 * of a delete-one jackknife over regions, halotools' tpcf_jackknife and pycorr's jackknife estimators;
 * pmesh_amd.pairlabels).  They are flag bits above the base modes: the valid modes are PMX_PAIRS_SPLIT | m (16 .. 20)
 * and PMX_PAIRS_JACKKNIFE | m (32 .. 36), m one of the base modes PMX_PAIRS_1D, PMX_PAIRS_2D, PMX_PAIRS_PROJECTED,
 * PMX_PAIRS_2D_MIDPOINT and PMX_PAIRS_PROJECTED_MIDPOINT; 10 to 15, 21 to 31 and 37 to 127 are PMX_EINVAL, and so is
 * everything from 128 on but the two alignment modes 128 and 130 and the moments mode 517 described further below.
 *   shared    rows, wrapping, the minimum image, r2, q, the squared edges, the r-, mu- and pi-bin and the pimax cut are
 *             exactly those of the base mode m, with its ndim (1 to 3 for 1D, three dimensions otherwise), its los and
 *             its sub; all arithmetic in double, every operation rounded once, no contraction, no square root choosing
 *             a bin.  Summed over its label classes, npairs of a label mode equals npairs of the base mode on the same
 *             arguments, to the last count.
 *   columns   weight1 and weight2 are both required: pmx_vecs of 2 columns, (w, label), float or double, in ROW order,
 *             read through order1 / order2.  A wrong ncol, or a missing vec, is PMX_EINVAL.  A label is a non-negative
 *             integer value held exactly in the column's type.  A label that is negative, not finite, or out of range
 *             for the call is "no label": the kernel tests it with a comparison that is false for NaN; such a row never
 *             indexes anything and is never "the same" as any row.
 *   PMX_PAIRS_SPLIT, nbins = nr * nsub <= 1024, else PMX_EINVAL.  With kind = (a == c and a is a label) ? 1 : 0, per
 *             counted pair of weight w = w1_i * w2_j in bin b: npairs[kind * nbins + b] += 1, wnpairs[...] += w,
 *             rsum[...] += w * sqrt(q).  All three arrays have 2 * nbins entries.
 *   PMX_PAIRS_JACKKNIFE, K = (PMX_PAIRS_LABEL_SLOTS / nbins - 2) / 2 in integer division; K >= 1 is required, that is
 *             nbins <= 1024, else PMX_EINVAL.  A label is in range when it is below K.  K is fixed by nbins alone: the
 *             entry needs no further parameter and cannot be handed arrays that are too short.  npairs and wnpairs have
 *             (1 + 2 K) * nbins entries, in blocks of nbins: block 0 is `all`, block 1 + k is side[k], block 1 + K + k
 *             is same[k].  rsum has nbins entries and covers `all` only.  Per counted pair in bin b, with labels a
 *             (primary) and c (secondary): all[b] gets (1, w, w sqrt(q)); if a is in range, side[a][b] gets (1, w); if c
 *             is in range, side[c][b] gets (1, w), so a pair with a == c adds 2 and 2w (w + w, exact); if a == c and in
 *             range, same[a][b] gets (1, w).
 *   sums      all arrays are added to, never overwritten.  npairs is exact and depends on no decomposition or launch.
 *             The order of the double sums is unspecified, as in the base modes.
 *   self      the entry knows no row identity.  A self pair has r2 == 0 and a == c, and the caller removes it, as in the
 *             base modes: from kind 1 (from kind 0 for a row without a label); from all, twice from side[a] and once
 *             from same[a].
 *   LDS       the histogram of a workgroup holds a 32-bit count and one double per slot over PMX_PAIRS_LABEL_SLOTS
 *             slots (pmx_pairs_labels.hip): the "- 2" in K pays for the block of `all` and for its r-sum.
 *
 * The modes with intrinsic-alignment sums (the position-shape and shape-shape correlations omega(r), eta(r), w_g+(rp)
 * and w_++(rp): halotools-ia's ed_3d, ee_3d, gi_plus_projected, ii_plus_projected and their minus partners;
 * pmesh_amd.alignments).  PMX_PAIRS_ALIGN is a flag bit above the base modes: the valid modes are PMX_PAIRS_ALIGN |
 * PMX_PAIRS_1D (128) and PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED (130); 129, 131, 132, 128 | 16, 128 | 32 and everything
 * from 133 on (but the moments mode 517) are PMX_EINVAL.  Mode 128 shares everything below with PMX_PAIRS_1D, mode 130 with PMX_PAIRS_PROJECTED:
 *   shared    rows, wrapping, the minimum image dx_d (primary minus secondary), r2, q, the squared edges, the r-bin, the
 *             pi-bin, the pimax cut and the loop over windows of 2^23 secondaries; all arithmetic in double; every
 *             operation rounded once, no contraction; no square root chooses a bin.  npairs equals npairs of the base
 *             mode on the same arguments, to the last count.
 *   columns   weight1 and weight2 are both required: contiguous pmx_vecs in ROW order, float or double, read through
 *             order1 / order2.  A wrong ncol, or a missing vec, is PMX_EINVAL.  A set without shapes brings zeros.
 *   outputs   npairs and wnpairs have nbins = nr * nsub entries.  rsum has (1 + NS) * nbins entries: rsum[m * nbins + b];
 *             m = 0: sum w sqrt(q), as in the base mode; m = 1 .. NS: the sums below.  All are added to, never
 *             overwritten.  nbins <= PMX_PAIRS_ALIGN_MAX_BINS, else PMX_EINVAL.  The order of the double sums is
 *             unspecified; npairs is exact.
 *   per counted pair, with w = w1_i * w2_j:
 *   PMX_PAIRS_ALIGN | PMX_PAIRS_1D, ndim 2 or 3 (1 is PMX_EINVAL), nsub == 1, NS = 3.  The columns are (w, a_0 ..
 *             a_{ndim-1}): an orientation vector, not necessarily a unit vector.  With a the primary's vector and c the
 *             secondary's, each sum over d < ndim in ascending d: a2 = sum a_d a_d, c2 = sum c_d c_d, pa = sum dx_d a_d,
 *             pc = sum dx_d c_d, ac = sum a_d c_d.
 *             t1 = (r2 > 0 && a2 > 0) ? (pa * pa) / (a2 * r2) : 0: cos^2 between the primary's axis and the separation.
 *             t2 = (r2 > 0 && c2 > 0) ? (pc * pc) / (c2 * r2) : 0.
 *             t3 = (r2 > 0 && a2 > 0 && c2 > 0) ? (ac * ac) / (a2 * c2) : 0: cos^2 between the two axes.
 *             S1 += w * t1, S2 += w * t2, S3 += w * t3
 *   PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED, ndim 3, los in {0, 1, 2}, sub = piedges, NS = 6.  The columns are (w, g1, g2):
 *             the spin-2 ellipticity in the plane normal to los, referred to the axes A < B, the two axes other than
 *             los in ascending order; g1 > 0 is elongation along A, g2 > 0 along the diagonal A = B.  With rp2 = q:
 *             cc = dx_A * dx_A - dx_B * dx_B, ss = 2.0 * (dx_A * dx_B).
 *             p1 = rp2 > 0 ? (g1_i * cc + g2_i * ss) / rp2 : 0, x1 = rp2 > 0 ? (g1_i * ss - g2_i * cc) / rp2 : 0 for the
 *             primary; p2 and x2 the same with the secondary's columns (the direction is spin-2: the reversed
 *             separation gives the same cc and ss).
 *             S1 += w * p1, S2 += w * p2, S3 += (w * p1) * p2, S4 += (w * x1) * x2, S5 += w * x1, S6 += w * x2
 *             p > 0: the shape points along the projected separation (radial alignment); x is the 45 degree
 *             component, whose means vanish by parity.  No trigonometric call and no square root beyond the base
 *             mode's.
 *   self      a pair with r2 == 0 (rp2 == 0) adds nothing to S1 .. S_NS: a self pair (one set passed as both) is inert
 *             there, and the caller subtracts it from npairs[0] and wnpairs[0] as in the base modes.
 *   scaling   a vector scaled by a power of two changes no bit of any sum of mode 128, and neither does a -> -a.  The
 *             products a2 * r2 and a2 * c2 must neither overflow nor underflow: finite, sanely scaled columns are the
 *             caller's business.
 *   LDS       the histogram of a workgroup holds a 32-bit count and 2 + NS doubles per bin (pmx_pairs_align.hip): 44 KB
 *             in mode 128, 68 KB in mode 130 at PMX_PAIRS_ALIGN_MAX_BINS bins.
 *
 * The mode with moment sums per primary row (the inertia tensor, axis ratios and major axis, the centre-of-mass offset,
 * the velocity dispersion, the angular momentum and the spin of the sources inside spheres about every centre: the
 * shape and spin columns of a halo catalogue; pmesh_amd.moments).  PMX_PAIRS_MOMENTS is a flag bit above the row mode:
 * the only valid mode is PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS (517).  512 alone, 512 | m for every other m in 0 .. 7
 * and 512 combined with 16, 32 or 128 are PMX_EINVAL.  ndim 2 or 3 (1 is PMX_EINVAL), nsub == 1, sub == NULL.
 *   shared    rows, wrapping, the minimum image, the arrays in the caller's row order that are added to, the windows of
 *             2^23 secondaries and the absent row identity are those of PMX_PAIRS_1D_ROWS.  For the primary row i and
 *             the secondary j: dx_d is what the row mode forms, centre minus source, minimum image; q = sum_d dx_d^2
 *             from 0 in ascending d, in double, every operation rounded once, no contraction; s_d = -dx_d (exact) is
 *             the source as seen from the centre.
 *   columns   weight1 is required: 2 columns (w_i, s2_i), s2_i the square of the centre's scale, finite and positive
 *             (the caller's business: a row with another s2 counts nothing or nonsense, and indexes nothing).  weight2
 *             is required: 1 column (m_j), or 1 + ndim columns (m_j, v_0 .. v_{ndim-1}).  Float or double, in ROW order,
 *             read through order1 / order2.  Any other column count, or a missing vec, is PMX_EINVAL.
 *   bins      the edges of row i are E_k = e2[k] * s2_i, one rounding each.  The pair is in bin k when E_k <= q <
 *             E_{k + 1}; it is not counted when q < E_0 or q >= E_nr: the comparisons of the base modes on E in place
 *             of e2.  With s2_i == 1.0 the bins are bit for bit those of PMX_PAIRS_1D_ROWS.
 *   limit     nr <= PMX_PAIRS_MOMENTS_MAX_BINS, else PMX_EINVAL.
 *   sums      per row i and bin b, with m = w_i * m_j (one rounding): npairs[i * nr + b] += 1 (exact, as in the row
 *             modes); wnpairs[i * nr + b] += m; rsum[(i * nr + b) * NS + k] += the k-th of, in this order,
 *               m * sqrt(q)
 *               m * s_d, d ascending
 *               m * s_a * s_b for a <= b, in the order 00, 01, 02, 11, 12, 22 (ndim 2: 00, 01, 11): NT = ndim (ndim +
 *                 1) / 2 of them
 *               the reduced tensor in the same order, (m * s_a * s_b) / q, the term 0 where q == 0
 *             and, where weight2 has velocities,
 *               m * v_d, d ascending
 *               m * (sum_d v_d^2)
 *               m * (s x v): (s_1 v_2 - s_2 v_1, s_2 v_0 - s_0 v_2, s_0 v_1 - s_1 v_0) in three dimensions, NL = 3;
 *                 s_0 v_1 - s_1 v_0 in two, NL = 1.
 *             NS = 1 + ndim + 2 NT without velocities and ndim + 1 + NL more with them: 16 or 23 doubles per (row, bin)
 *             in three dimensions, 9 or 13 in two.  rsum has NS * n1 * nr entries.  The double sums have no fixed
 *             order; within a term the operations may be contracted or regrouped (the kernel forms m / q once per
 *             pair): a term carries at most four roundings.  A source that coincides with a centre is a pair at q ==
 *             0: counted in bin 0 when e2[0] == 0, with s == 0 and its reduced term 0.
 *   LDS       one wave per primary row keeps its scaled edges and its histogram, a 32-bit count and 1 + NS doubles per
 *             slot over PMX_PAIRS_MOMENTS_MAX_BINS slots (bins x copies), in LDS: 51 KB per workgroup of four waves at
 *             23 sums (pmx_pairs_moments.hip). */
#define PMX_PAIRS_MAX_BINS 4096         /* nr, nr * nmu or nrp * npi of one call (nbodykit's habitual 40 x 100 fits) */
#define PMX_PAIRS_1D 0                   /* `mode`: bins of r */
#define PMX_PAIRS_2D 1                   /* bins of (r, mu) */
#define PMX_PAIRS_PROJECTED 2            /* bins of (rp, pi) */
#define PMX_PAIRS_2D_MIDPOINT 3          /* bins of (s, mu), the line of sight from the box centre to the pair's midpoint */
#define PMX_PAIRS_PROJECTED_MIDPOINT 4   /* bins of (rp, pi), the same line of sight */
#define PMX_PAIRS_1D_ROWS 5              /* bins of r, one histogram per primary row */
#define PMX_PAIRS_PROJECTED_ROWS 6       /* bins of (rp, pi) about the axis los, one histogram per primary row */
#define PMX_PAIRS_ROWS_MAX_BINS 256      /* nr * nsub of one call in the two row modes */
#define PMX_PAIRS_1D_VELOCITY 7          /* bins of r; radial pairwise velocity */
#define PMX_PAIRS_PROJECTED_VELOCITY 8   /* bins of (rp, pi) about the axis los; line-of-sight pairwise velocity */
#define PMX_PAIRS_1D_LOS 9               /* bins of r; one line-of-sight scalar per row, observer at the box centre */
#define PMX_PAIRS_VELOCITY_MAX_BINS 1024 /* nr * nsub of one call in these three modes */
#define PMX_PAIRS_SPLIT      16   /* | base mode 0..4: pairs apart by "same label" / "not" */
#define PMX_PAIRS_JACKKNIFE  32   /* | base mode 0..4: all pairs, and per label those touching it and those inside it */
#define PMX_PAIRS_LABEL_SLOTS 4096
#define PMX_PAIRS_ALIGN      128  /* | PMX_PAIRS_1D (128) or PMX_PAIRS_PROJECTED (130): intrinsic-alignment sums */
#define PMX_PAIRS_ALIGN_MAX_BINS 1024    /* nr * nsub of one call in these two modes */
#define PMX_PAIRS_MOMENTS    512  /* | PMX_PAIRS_1D_ROWS (517): moment sums per primary row, bins in units of its scale */
#define PMX_PAIRS_MOMENTS_MAX_BINS 64    /* nr of one call in that mode */

/* npairs[b], wnpairs[b], rsum[b] += the sums over the pairs of bin b (DEVICE int64 / double / double arrays of
 * nr * nsub entries; the caller zeroes them, or keeps adding).  One entry, one kernel.
 * The primaries: spos1 (DEVICE double (n1, ndim) contiguous), order1 and cell_of1 are what pmx_fof_cells / pmx_fof_fill
 * left of pos1: the wrapped rows in cell order, the row of every slot, the flat cell of every ROW.  The secondaries: spos2,
 * order2, cell_start2 (prod(ncell) + 1 entries) likewise of pos2, on the SAME grid (ncell, periodic, boxsize as passed
 * to pmx_fof_cells for both).  The same arrays may be passed for both sets.  The cell_start of the primaries is not
 * needed: one lane per slot of the primaries walks the 3^ndim neighbouring cells of its row in the secondaries.
 * weight1 / weight2: one column of n1 / n2 floats or doubles in ROW order (read through order1 / order2), NULL for 1.
 * With both NULL no weight is read and wnpairs[b] += (double)(the count).
 * e2: DEVICE double, nr + 1 entries.  sub: DEVICE double, nsub + 1 entries, m2 (2D, 2D_MIDPOINT), piedges (projected)
 * or piedges^2 (PROJECTED_MIDPOINT); NULL and nsub = 1 in the mode 1D.  los is ignored in the mode 1D and in the two
 * midpoint modes, whose kernels (pmx_pairs_survey.hip) are launched from this entry like the others, as are those of
 * the two row modes (pmx_pairs_rows.hip), whose three arrays have n1 * nr * nsub entries, and those of the three
 * velocity modes (pmx_pairs_vel.hip), whose weight1 / weight2 have 1 + ndim or 2 columns and whose rsum has
 * 4 * nr * nsub entries, and those of the modes by row labels (pmx_pairs_labels.hip), whose weight1 / weight2 have 2
 * columns and whose arrays have the lengths given above, and those of the two alignment modes (pmx_pairs_align.hip),
 * whose weight1 / weight2 have 1 + ndim or 3 columns and whose rsum has 4 or 7 times nr * nsub entries.
 * The bins are accumulated in a histogram per workgroup in LDS (32-bit counts, double sums); a workgroup makes one global
 * atomic per array and non-zero bin at its end, never one per pair.  No workgroup is given more than 2^31 pairs per
 * launch: above 2^23 secondaries the entry launches once per window of 2^23 slots of the secondaries.  Reads 8 ndim + 8 bytes per slot of the primaries and 8 ndim (+ 4 + elsize with weights)
 * per visited pair, the latter from cache: the lanes of a wave share their neighbouring cells. */
int pmx_pair_counts(int32_t ndim, int32_t mode, int32_t los, int64_t n1, const double *spos1, const int32_t *order1,
                    const int32_t *cell_of1, const pmx_vec *weight1, int64_t n2, const double *spos2,
                    const int32_t *order2, const int32_t *cell_start2, const pmx_vec *weight2, const int64_t *ncell,
                    int32_t periodic, const double *boxsize, int32_t nr, const double *e2, int32_t nsub,
                    const double *sub, int64_t *npairs, double *wnpairs, double *rsum, void *stream);

/* ---- multipoles of the three-point function of particles (what nbodykit's SimulationBox3PCF does on the host with a
 * kd-tree; pmesh_amd.threept) ------------------------------------------------------------------------------------------
 * The rule.
 *   rows     pos and pos2 are (n, 3) rows, float or double (a float is widened exactly), wrapped and differenced as for
 *            the pair counts: FoF's wrap, then the minimum image of the wrapped rows.  All arithmetic is in double;
 *            r2 = dx_0^2 + dx_1^2 + dx_2^2, summed in that order.  Three dimensions only.
 *   bins     e2[k] = edges[k] * edges[k] is formed by the caller, edges as for the pair counts.  Row j is a neighbour of
 *            i in bin b when e2[b] <= r2 < e2[b + 1].  A pair with r2 == 0 is never a neighbour (the row itself, a
 *            coincident row): it has no direction.  The search radius is b = edges[nr], 2 b <= min_d L_d; nr is at most
 *            PMX_THREEPT_MAX_BINS.
 *   dir      r = sqrt(r2), u_d = dx_d / r.
 *   sums     with N_i(b) the neighbours of primary i in bin b, taken from the secondaries, for l = 0 .. lmax
 *                zeta_l[b1, b2] = sum_i w_i sum_{j in N_i(b1)} sum_{k in N_i(b2)} w_j w_k P_l(u_ij . u_ik)
 *            the term j == k (b1 == b2) included; so that a caller can remove it: diag[b] = sum_i w_i sum_{j in N_i(b)}
 *            w_j^2 (P_l(1) = 1: the same for every l), npairs[b] = sum_i |N_i(b)| (int64, exact), wpairs[b] = sum_i w_i
 *            sum_{j in N_i(b)} w_j.
 *   how      per primary A_{l,c}(b) = sum_j w_j Y_{l,c}(u_ij) over the 2 l + 1 real components, for m = 0 .. l,
 *            Y = N_lm Q_l^m(u_z) Re / Im (u_x + i u_y)^m with N_lm = sqrt(eps_m (l - m)! / (l + m)!), eps_0 = 1, eps_m =
 *            2 otherwise; Q_l^m = P_l^m / sin^m, a polynomial in u_z, from Q_m^m = (2 m - 1)!!, Q_{m+1}^m = (2 m + 1) z
 *            Q_m^m and (l - m) Q_l^m = (2 l - 1) z Q_{l-1}^m - (l + m - 1) Q_{l-2}^m; (u_x + i u_y)^m by repeated
 *            complex multiplication.  By the addition theorem sum_c A_{l,c}(b1) A_{l,c}(b2) is the double sum of P_l,
 *            and zeta_l += w_i times it (Slepian & Eisenstein 2015: O(N neighbours), not O(N neighbours^2)).
 *            N_00 Q_0^0 = 1 exactly: with unit weights zeta_0 is a sum of integers, exact below 2^53.
 *   forms    the entry knows no row identity: a caller passes one set as both for the auto form.  The order of the
 *            double sums is unspecified; npairs, and zeta_0 with unit weights, never vary. */
#define PMX_THREEPT_MAX_ELL 10           /* the largest multipole l of one call */
#define PMX_THREEPT_MAX_BINS 32          /* the most radial bins nr of one call */

/* zeta[l, b1, b2], diag[b], wpairs[b], npairs[b] += the sums of the rule (DEVICE double (lmax + 1, nr, nr), double (nr),
 * double (nr), int64 (nr); the caller zeroes them, or keeps adding); the sums go into zeta[l, b1 >= b2] and the entry
 * ends by copying them to zeta[l, b2, b1]: zeta is symmetric to the last bit.  One entry, one kernel and that copy.
 * The primaries (spos1, order1, cell_of1), the secondaries (spos2, order2, cell_start2), the weights and the grid
 * (ncell, periodic, boxsize; three axes) are those of pmx_pair_counts; e2: DEVICE double, nr + 1 entries; lmax in
 * 0 .. PMX_THREEPT_MAX_ELL.
 * One workgroup takes a run of consecutive slots of the primaries and treats them one after another: its lanes stride
 * over the slots of the 27 neighbouring cells, compact the neighbours into a chunk in LDS, evaluate w Y for a chunk
 * at a time and add it into A[bin][component] in LDS with one owner per word; after the walk every lane adds w_i sum_c
 * A[b1][c] A[b2][c] into the outputs (l, b1 >= b2) it keeps in registers for the whole run.  One global atomic per
 * workgroup and non-zero output at its end.  No 32-bit counter spans more than one primary.  Reads 28 bytes per
 * primary and 24 (+ 4 + elsize with weight2) per visited pair, the latter from cache. */
int pmx_threept_multipoles(int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1,
                           const pmx_vec *weight1, int64_t n2, const double *spos2, const int32_t *order2,
                           const int32_t *cell_start2, const pmx_vec *weight2, const int64_t *ncell, int32_t periodic,
                           const double *boxsize, int32_t nr, const double *e2, int32_t lmax, double *zeta,
                           double *diag, double *wpairs, int64_t *npairs, void *stream);

/* ---- the short-range pair force of particles (the tree half of MP-Gadget's TreePM force, as a P3M sum over the cell
 * grid; pmesh_amd.shortrange) ---------------------------------------------------------------------------------------
 * The rule.
 *   rows     pos (primaries) and pos2 (sources) are (n, 3) rows, float or double (a float is widened exactly), wrapped
 *            and differenced as for the pair counts: FoF's wrap, then dx_d = x_i,d - x_j,d, the minimum image of the
 *            wrapped rows.  All arithmetic is in double; r2 = dx_0^2 + dx_1^2 + dx_2^2, summed in that order.  Three
 *            dimensions only.
 *   cut      source j is a neighbour of primary i when 0 < r2 < rc2, rc2 = r_cut * r_cut formed by the caller; no
 *            square root decides it.  r_cut is finite, positive and 2 r_cut <= min_d L_d.  A pair with r2 == 0 (a row
 *            with itself, coincident rows) contributes nothing: the entry needs no row identity, and a caller that
 *            passes one set as both has nothing to correct.
 *   force    r = sqrt(r2), u = r / (2 r_split), s2 = r2 + eps2 (eps2 = softening^2, Plummer),
 *                fac = erfc(u) + (2 / sqrt(pi)) u exp(-u^2)
 *                acc_i,d = -G sum_j m_j dx_d fac / (s2 sqrt(s2))
 *                pot_i   = -G sum_j m_j erfc(u) / sqrt(s2)
 *                neighbours_i = the number of neighbours (int64, exact)
 *            erfc and exp are the device's double functions, evaluated in closed form for every pair.  The sum of this
 *            force and a mesh force filtered by exp(-k^2 r_split^2) (pmx_transfer.gauss_r = sqrt(2) r_split) is
 *            Newton's.
 *   sums     the order of the double sums is unspecified: their last bits may vary; neighbours never varies. */

/* acc[i, :], pot[i], neighbours[i] = the sums of the rule for row i of the primaries (DEVICE double (n1, 3), double
 * (n1) or NULL, int64 (n1) or NULL), in ROW order (written through order1); they are overwritten, not added to.
 * The primaries (spos1, order1, cell_of1), the sources (spos2, order2, cell_start2) and the grid (ncell, periodic,
 * boxsize; three axes) are those of pmx_pair_counts; the same arrays may be passed for both sets.  mass2: one column of
 * n2 floats or doubles in ROW order (read through order2), NULL for 1.  G, r_split > 0, rc2 > 0 and eps2 >= 0 are
 * finite.  One entry, one kernel: one wave per slot of the primaries strides over the slots of the 27 neighbouring
 * cells, compacts the pairs inside the cut into a ring in LDS of its own and evaluates the force 64 pairs at a time;
 * a fixed shuffle tree sums the lanes.  No atomics, no counter that spans more than one primary.  Reads 28 bytes and
 * writes 24 (+ 8 + 8) per primary, reads 24 per visited pair (+ 4 + elsize per neighbour with masses), the latter from
 * cache. */
int pmx_short_range(int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1, int64_t n2,
                    const double *spos2, const int32_t *order2, const int32_t *cell_start2, const pmx_vec *mass2,
                    const int64_t *ncell, int32_t periodic, const double *boxsize, double G, double r_split,
                    double rc2, double eps2, double *acc, double *pot, int64_t *neighbours, void *stream);

/* ---- the k nearest neighbours of particles (what callers do with a kd-tree on the host: nbodykit's KDDensity,
 * MP-Gadget's smoothing lengths, the kNN-CDF statistics; pmesh_amd.knn) -----------------------------------------------
 * The rule.
 *   rows        pos (primaries) and pos2 (sources) are (n, ndim) rows, ndim = 1, 2 or 3, float or double (a float is
 *               widened exactly), wrapped and differenced as for the pair counts: FoF's wrap, then dx_d = x_i,d - x_j,d,
 *               the minimum image of the wrapped rows.  All arithmetic is in double, every operation rounded once; r2 =
 *               sum_d dx_d^2, accumulated in the order d = 0, 1, 2.
 *   candidates  source j is a candidate of primary i when r2 < rmax2, rmax2 = rmax * rmax formed by the caller; no
 *               square root decides anything.  rmax is finite, positive and 2 rmax <= min_d L_d.
 *   result      dist2[i, :] are the k smallest candidate r2 of row i, ascending, +inf where there are fewer candidates.
 *               The multiset of the k smallest values is unique: dist2 is defined bit for bit and depends on no
 *               decomposition, launch or search schedule.  index[i, c] is a source whose r2 to row i equals dist2[i, c],
 *               -1 where that is inf; the indices of a row are distinct; among sources tied in r2 the one named is
 *               unspecified: the indices are witnesses, not a canonical order.  found[i] is the number of finite
 *               columns.
 *   auto form   the entry knows no row identity: a caller that searches a set in itself asks for k + 1 and removes the
 *               column that names the row itself (r2 == 0 exactly), or the last column where it is not named. */
#define PMX_KNN_MAX_K 64                 /* the most neighbours k of one call: one per lane of a wave */

/* dist2[i, :], index[i, :], count[i] = the k smallest r2 < r2max of row i of the primaries, ascending and padded with
 * +inf; the LOCAL rows of those sources (through order2), -1 where inf; the exact number of sources with r2 < r2max,
 * not capped at k (DEVICE double (n1, k), int32 (n1, k) or NULL, int64 (n1) or NULL), in ROW order (written through
 * order1); they are overwritten.  One launch is a fixed-radius top-k over the 3^ndim neighbouring cells: r2max is the
 * squared radius of this launch, and the cells have a side of at least that radius.  count[i] >= k says that the k
 * nearest of row i all lie inside the radius; a caller that wants the k nearest within a larger rmax launches again
 * with a larger radius for the other rows (pmesh_amd.knn.knn: the radius doubles).
 * The primaries (spos1, order1, cell_of1), the sources (spos2, order2, cell_start2) and the grid (ncell, periodic,
 * boxsize; ndim axes) are those of pmx_pair_counts; the same arrays may be passed for both sets.  1 <= k <=
 * PMX_KNN_MAX_K.  One entry, one kernel: one wave per slot of the primaries strides over the slots of the neighbouring
 * cells; count is the sum of the ballots' populations; a candidate is kept when r2 < tau, tau = r2max until the wave's
 * list holds k finite entries and their k-th smallest from then on; what is kept is compacted into a ring in LDS of the
 * wave's own and merged 64 entries at a time into the best list (one entry per lane, ascending) by a bitonic sort, a
 * min with the reversed list and a bitonic merge, all lane exchanges.  No atomics, no counter that spans more than one
 * primary.  Reads 4 + 4 + 8 ndim bytes and writes 12 k + 8 per primary, reads 8 ndim per visited source, the latter
 * from cache. */
int pmx_knn(int32_t ndim, int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1, int64_t n2,
            const double *spos2, const int32_t *order2, const int32_t *cell_start2, const int64_t *ncell,
            int32_t periodic, const double *boxsize, double r2max, int32_t k, double *dist2, int32_t *index,
            int64_t *count, void *stream);

/* Where the master seed stream of pmx_whitenoise runs (pmesh/_whitenoise_generics.h:73-93: one RANLUX stream walked in
 * rings over the (i, j) plane, one seed per column): 0 (default) one host core + a copy of 8 bytes per local column;
 * 1 one device thread (no copy, no wait; a sequential chain: ~35 x slower than the host core).  Same tables bit for bit. */
int pmx_whitenoise_master(int32_t on_device);
/* ---- white noise (the step before the cycle: initial conditions) -------------------------
 * pmesh.whitenoise.generate for 3-d meshes (pmesh/_whitenoise.pyx:25-45,
 * _whitenoise_imp.c:75-105, _whitenoise_generics.h:29-238; pm.py:1656-1696): fills the local
 * block [start, start+size) of the spectrum with the Gadget / N-GenIC compatible Gaussian (unitary = 0) or fixed-amplitude
 * (unitary = 1) Hermitian white noise of `seed`: every (i, j) column has its own RANLUX stream
 * seeded from a master stream walked in N-GenIC's ring order, so the result is independent
 * of the decomposition and the large scales do not change with the mesh size.
 * canvas: complex64 (elsize 8) or complex128 (elsize 16), byte strides.  The (i, j) seed table
 * is built on the host (a sequential stream of N0*N1 draws) and the columns are filled on the
 * device, one thread per column and generator.  A block that reaches beyond the Nyquist plane
 * (start[2] + size[2] > nmesh[2]/2 + 1: complex-to-complex meshes) gets the full spectrum. */
int pmx_whitenoise(uint32_t seed, int32_t unitary, const int64_t *nmesh, const int64_t *start,
                   const int64_t *size, const int64_t *strides, int32_t elsize, void *canvas,
                   void *stream);

/* ---- synthetic inputs for bench.py ------------------------ */
/* lattice + hashed jitter; writes pos (npart,3) for lattice ids [g0, g0+npart) */
int pmx_synth_uniform(const pmx_vec *pos, int64_t nlat, double boxsize, uint64_t seed, int64_t g0,
                      int64_t npart, void *stream);
/* lattice + plane-wave Zel'dovich displacement; modes: nmodes x 8 doubles on the
 * HOST (nx, ny, nz, dirx, diry, dirz, amplitude, phase) */
int pmx_synth_clustered(const pmx_vec *pos, int64_t nlat, double boxsize, const double *modes,
                        int32_t nmodes, double shift, int64_t g0, int64_t npart, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PMESH_AMD_H */
