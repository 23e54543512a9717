// pmx_bispec.hip — the two kernels of the binned bispectrum (include/pmesh_amd.h: pmx_bispec_shells,
// pmx_bispec_reduce; pmesh_amd/bispectrum.py).
//
// Replaces the composition of a bskit-style estimator out of field operations: one masked copy of the spectrum per
// shell (ComplexField.apply) and, after the c2r of every shell, one (D_i * D_j * D_l).sum() per triangle bin — which
// reads every shell field from HBM once per triangle it takes part in.
//
// shells_kernel streams: one read of the mode (none in unit mode), nb writes, one thread per mode in memory order.
// |k| and the shell of a mode are computed as pmx_power.hip computes them (k_divided and sinc_pow of pmx_block_dev.h,
// the sum of mode_k, find_bin of pmx_power_dev.h), so a mode lands in the same shell here and in pmx_power_project.
//
// reduce_kernel: a workgroup of sixteen waves stages a chunk of 64 K cells x nb shells in LDS as doubles (the only
// read of the fields; every thread loads, a cell for every second, fourth or eighth shell).  Then its lanes own cells
// (K each, the same K for every shell) and its waves share out the triangle list in equal contiguous parts, walked in
// groups of 64.  The list is uniform over a wave: a wave takes the triple of a triangle with readlane, forms the pair
// product D_i D_j of its lanes' cells in registers (kept while consecutive triangles share (i, j): the list of
// bispectrum.py is sorted), reads D_l from LDS — conflict-free, lane-consecutive addresses —, sums its K cells and
// reduces over the wave with DPP row operations and four readlanes (no LDS traffic).  Lane t of the wave keeps the
// sum of the group's triangle t; after the group the 64 sums are added, one coalesced read-modify-write, into the
// workgroup's own row of a [nwg][ntri] buffer.  sum_kernel then adds the rows in fixed order into acc: chunk ->
// workgroup -> row are all fixed by the shapes, so the result is the same bit for bit from run to run.
// Measured forms: four waves per workgroup, runs of four triangles of one pair in flight at once, and the
// sums of sixteen triangles added across the lanes by one transposing butterfly were all slower than this one.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"
#include "pmx_power_dev.h"   // find_bin, guess

namespace pmx {

// ---- shells ----------------------------------------------------------------------------------------------------------

struct BShells {
    int32_t nb, deconv_pow, unit;
};

struct BPtrs {
    char *p[PMX_BISPEC_MAX_SHELLS];
};

template <typename T>
__global__ void __launch_bounds__(256) shells_kernel(BlockGeom g, BShells p, const char *__restrict__ a, BlockStr as,
                                                     BPtrs out, BlockStr os, const double *__restrict__ kedges)
{
    __shared__ double ke[PMX_BISPEC_MAX_SHELLS + 1];
    for (int i = threadIdx.x; i <= p.nb; i += 256) ke[i] = kedges[i];
    __syncthreads();
    const int nb = p.nb;
    const double ke0 = ke[0], kinv = nb / (ke[nb] - ke[0]);
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3], ww[3];
        const double kmag = sqrt(wavevector<true>(g, idx, kk, ww));
        int j = -1;
        if (kmag >= ke0 && kmag < ke[nb]) j = find_bin(ke, nb, kmag, guess(kmag, ke0, kinv));
        double re = 1, im = 0;
        if (!p.unit && j >= 0) {
            CLoad<T>::get(a + as.off(idx), re, im);
            if (p.deconv_pow) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    if (d >= g.ndim) continue;
                    const double sp = sinc_pow(ww[d], p.deconv_pow);
                    re /= sp;
                    im /= sp;
                }
            }
        }
        const int64_t off = os.off(idx);
        for (int s = 0; s < nb; s++) {
            const bool mine = s == j;
            CLoad<T>::put(out.p[s] + off, mine ? re : 0.0, mine ? im : 0.0);
        }
    }
}

#undef PMX_BLOCK_LOOP

// ---- reduce ----------------------------------------------------------------------------------------------------------

constexpr int BWG = 1024;                     // threads of a reduce workgroup: sixteen waves share a staged chunk
constexpr int BMAX_WG = 512;                  // rows of the partial buffer at most

struct BFields {
    const char *p[PMX_BISPEC_MAX_SHELLS];
};

struct BReduce {
    int64_t shape[3], s[3];                   // logical shape and common byte strides of the real blocks
    int64_t ncells, nchunks;
    int32_t nb, ntri;
};

template <int CTRL> __device__ __forceinline__ double dpp_move(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double lane_value(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the sum of v over the 64 lanes, the same value (and the same order of additions) in every lane: within rows of 16
// lanes by quad permutes and row rotations, then the four row sums in sequence
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_move<0xB1>(v);                   // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);                   // quad_perm [2, 3, 0, 1]
    v += dpp_move<0x124>(v);                  // row_ror 4
    v += dpp_move<0x128>(v);                  // row_ror 8
    return ((lane_value(v, 0) + lane_value(v, 16)) + lane_value(v, 32)) + lane_value(v, 48);
}

// K cells per lane: a chunk holds CH = 64 K cells; lane's cells are 2 lane, 2 lane + 1 of every run of 128 (one
// 16-byte LDS read per pair)
template <typename T, int K>
__global__ void __launch_bounds__(BWG) reduce_kernel(BReduce g, BFields f, const int32_t *__restrict__ tri,
                                                     double *__restrict__ part)
{
    extern __shared__ __align__(16) double sm[];   // [nb][CH]
    constexpr int CH = 64 * K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = g.nb, ntri = g.ntri;
    // this wave's part of the list (equal parts: the time of a chunk is that of the longest part)
    const int per = (ntri + BWG / 64 - 1) / (BWG / 64);
    const int w0 = min(ntri, wv * per), w1 = min(ntri, w0 + per);
    double *row = part + (int64_t)blockIdx.x * ntri;
    const int64_t n12 = g.shape[1] * g.shape[2];

    bool first = true;
    for (int64_t chunk = blockIdx.x; chunk < g.nchunks; chunk += gridDim.x) {
        // stage: thread tid takes cell tid mod CH for every (BWG / CH)-th shell; one offset serves all of them
        {
            const int c = tid % CH;
            const int64_t n = chunk * CH + c;
            const bool in = n < g.ncells;
            int64_t off = 0;
            if (in) {
                const int64_t i0 = n / n12, r = n - i0 * n12;
                const int64_t i1 = r / g.shape[2], i2 = r - i1 * g.shape[2];
                off = i0 * g.s[0] + i1 * g.s[1] + i2 * g.s[2];
            }
#pragma unroll 8
            for (int s = tid / CH; s < nb; s += BWG / CH) sm[s * CH + c] = in ? (double)*(const T *)(f.p[s] + off) : 0.0;
        }
        __syncthreads();

        for (int t0 = w0; t0 < w1; t0 += 64) {
            const int nt = min(64, w1 - t0);
            const bool on = lane < nt;
            int ti = 0, tj = 0, tl = 0;
            double mine = 0;
            if (on) {
                ti = tri[3 * (t0 + lane)];
                tj = tri[3 * (t0 + lane) + 1];
                tl = tri[3 * (t0 + lane) + 2];
                if (!first) mine = row[t0 + lane];
            }
            int pi = -1, pj = -1;
            double p[K];
            for (int t = 0; t < nt; t++) {
                const int i = __builtin_amdgcn_readlane(ti, t), j = __builtin_amdgcn_readlane(tj, t),
                          l = __builtin_amdgcn_readlane(tl, t);
                // (a triple that names no shell reads nothing: its sum is NaN)
                if ((unsigned)i >= (unsigned)nb || (unsigned)j >= (unsigned)nb || (unsigned)l >= (unsigned)nb) {
                    if (lane == t) mine = NAN;
                    continue;
                }
                if (i != pi || j != pj) {
                    const double2 *di = (const double2 *)(sm + i * CH) + lane, *dj = (const double2 *)(sm + j * CH) + lane;
#pragma unroll
                    for (int k = 0; k < K / 2; k++) {
                        const double2 x = di[k * 64], y = dj[k * 64];
                        p[2 * k] = x.x * y.x;
                        p[2 * k + 1] = x.y * y.y;
                    }
                    pi = i;
                    pj = j;
                }
                const double2 *dl = (const double2 *)(sm + l * CH) + lane;
                double s = 0;
#pragma unroll
                for (int k = 0; k < K / 2; k++) {
                    const double2 z = dl[k * 64];
                    s += p[2 * k] * z.x;
                    s += p[2 * k + 1] * z.y;
                }
                s = wave_sum(s);
                if (lane == t) mine += s;
            }
            if (on) row[t0 + lane] = mine;
        }
        first = false;
        __syncthreads();
    }
}

// acc[t] += the partial rows in sequence
__global__ void __launch_bounds__(256) sum_kernel(const double *__restrict__ part, int nrows, int ntri,
                                                  double *__restrict__ acc)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntri) return;
    double s = 0;
    for (int r = 0; r < nrows; r++) s += part[(int64_t)r * ntri + t];
    acc[t] += s;
}

// cells per lane for nb shells: the staged chunk takes up to 64 KB of LDS (two workgroups per CU)
static int cells_per_lane(int nb) { return nb <= 16 ? 8 : (nb <= 32 ? 4 : 2); }

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_bispec_shells(int32_t ndim, int32_t elsize, int32_t nb, int32_t deconv_pow, int32_t unit,
                                 const void *a, const int64_t *a_strides, void *const *out,
                                 const int64_t *out_strides, const int64_t *shape, const int64_t *start,
                                 const int64_t *nmesh, const double *boxsize, const double *kedges, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && out && out_strides && shape && start && nmesh && boxsize && kedges,
                PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(unit || (a && a_strides), PMX_EINVAL, "the field is needed unless unit is set");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nb >= 1, PMX_EINVAL, "nb must be >= 1");
    PMX_REQUIRE(nb <= PMX_BISPEC_MAX_SHELLS, PMX_EUNSUPPORTED, "nb above PMX_BISPEC_MAX_SHELLS");
    PMX_REQUIRE(deconv_pow >= 0, PMX_EINVAL, "deconv_pow must be >= 0");
    // memory order by decreasing stride of the outputs, axes of extent 1 slowest
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides, AXES_UNIT_SLOWEST);
    for (int d = 0; d < 3; d++) PMX_REQUIRE(g.shape[d] >= 0 && g.nmesh[d] >= 1, PMX_EINVAL, "bad shape");
    const BShells p = {nb, deconv_pow, unit ? 1 : 0};
    BPtrs o;
    for (int s = 0; s < PMX_BISPEC_MAX_SHELLS; s++) {
        o.p[s] = s < nb ? (char *)out[s] : nullptr;
        PMX_REQUIRE(s >= nb || o.p[s], PMX_EINVAL, "output pointer");
    }
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr as = make_str(ndim, unit ? nullptr : a_strides), os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        shells_kernel<T><<<grid, 256, 0, st>>>(g, p, (const char *)a, as, o, os, kedges);
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_bispec_reduce(int32_t ndim, int32_t elsize, int32_t nb, const void *const *fields,
                                 const int64_t *strides, const int64_t *shape, int32_t ntri, const int32_t *triangles,
                                 double *acc, double *work, int64_t work_doubles, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && fields && strides && shape && triangles && acc && work, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nb >= 1 && ntri >= 0, PMX_EINVAL, "nb must be >= 1, ntri >= 0");
    PMX_REQUIRE(nb <= PMX_BISPEC_MAX_SHELLS, PMX_EUNSUPPORTED, "nb above PMX_BISPEC_MAX_SHELLS");
    PMX_REQUIRE(ntri <= PMX_BISPEC_MAX_TRIANGLES, PMX_EUNSUPPORTED, "ntri above PMX_BISPEC_MAX_TRIANGLES");
    PMX_REQUIRE(work_doubles >= ntri, PMX_EINVAL, "work holds fewer than ntri doubles");
    BReduce g;
    BFields f;
    g.ncells = 1;
    for (int d = 0; d < 3; d++) {
        // (leading axes of extent 1 when ndim < 3: the cell walk is row-major over the logical shape)
        const int s = d - (3 - ndim);
        g.shape[d] = s >= 0 ? shape[s] : 1;
        g.s[d] = s >= 0 ? strides[s] : 0;
        PMX_REQUIRE(g.shape[d] >= 0, PMX_EINVAL, "bad shape");
        g.ncells *= g.shape[d];
    }
    for (int s = 0; s < PMX_BISPEC_MAX_SHELLS; s++) {
        f.p[s] = s < nb ? (const char *)fields[s] : nullptr;
        PMX_REQUIRE(s >= nb || f.p[s] || g.ncells == 0, PMX_EINVAL, "field pointer");
    }
    if (g.ncells == 0 || ntri == 0) return PMX_OK;
    const int K = cells_per_lane(nb);
    g.nchunks = (g.ncells + 64 * K - 1) / (64 * K);
    g.nb = nb;
    g.ntri = ntri;
    // work: the partial rows, one per workgroup
    double *part = work;
    int64_t nwg = work_doubles / ntri;
    if (nwg > BMAX_WG) nwg = BMAX_WG;
    if (nwg > g.nchunks) nwg = g.nchunks;
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        auto launch = [&](auto k) {
            constexpr int KC = decltype(k)::value;
            reduce_kernel<T, KC><<<(int)nwg, BWG, sizeof(double) * g.nb * 64 * KC, st>>>(g, f, triangles, part);
        };
        if (K == 8) launch(int_c<8>{});
        else if (K == 4) launch(int_c<4>{});
        else launch(int_c<2>{});
    });
    PMX_HIP_CHECK(hipGetLastError());
    sum_kernel<<<(ntri + 255) / 256, 256, 0, st>>>(part, (int)nwg, ntri, acc);
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
