// pmx_bispec_grad.hip — the two adjoint kernels of the binned bispectrum (include/pmesh_amd.h: pmx_bispec_pairsum,
// pmx_bispec_shells_vjp; pmesh_amd/bispectrum.py: bispectrum_vjp), next to pmx_bispec.hip as pmx_power_grad.hip is
// next to pmx_power.hip.
//
// Replaces the composition of the gradient out of field operations: one weighted product of two whole shell fields
// per (triangle, target shell) — three per triangle bin — and one masked, window-divided copy per shell.
//
// pairsum_kernel is the adjoint of reduce_kernel: G_s(x) = sum_e w_e D_p(x) D_q(x) over the entries e of shell s's
// range of a per-target list.  A workgroup of sixteen waves stages a chunk of 64 K cells x nb shells in LDS as doubles,
// exactly as reduce_kernel does (the only read of the fields).  After the barrier a wave owns one run of 128 cells of
// the chunk (lane's cells 2 lane and 2 lane + 1: one 16-byte LDS read per pair; the run is wv mod K / 2, the same for
// every shell, so a wave forms its two cell offsets once per chunk) and every (32 / K)-th target shell.  It keeps G_s
// of its two cells in registers while it walks shell s's entry range: the range is uniform over the wave, so entries
// are loaded 64 at a time, one per lane, and handed round with readlane; D_p is kept while consecutive entries share p
// (the host sorts the list).  G_s goes straight to global memory as T: no G array in LDS, no cross-lane reduction, no
// atomics, and one barrier more only before the next chunk is staged.  outs[s] may be fields[s]: a chunk is wholly
// staged before any of its cells is written, and no other workgroup touches these cells.  The sum of a cell runs in
// list order in one lane: the same bits from run to run.
//
// shells_vjp_kernel is the adjoint of shells_kernel: one thread per mode in memory order, |k|, the shell and the
// window as there (wavevector<true>, find_bin, sinc_pow, divided axis by axis), one read from the one spectrum the mode
// belongs to, one write.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"
#include "pmx_power_dev.h"   // find_bin, guess

namespace pmx {

struct BGIn {
    const char *p[PMX_BISPEC_MAX_SHELLS];
};

struct BGOut {
    char *p[PMX_BISPEC_MAX_SHELLS];
};

// ---- shells_vjp ------------------------------------------------------------------------------------------------------

template <typename T>
__global__ void __launch_bounds__(256) shells_vjp_kernel(BlockGeom g, int nb, int deconv_pow, BGIn in, BlockStr is,
                                                         char *out, BlockStr os, const double *__restrict__ kedges)
{
    __shared__ double ke[PMX_BISPEC_MAX_SHELLS + 1];
    for (int i = threadIdx.x; i <= nb; i += 256) ke[i] = kedges[i];
    __syncthreads();
    const double ke0 = ke[0], kinv = nb / (ke[nb] - ke[0]);
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3], ww[3];
        const double kmag = sqrt(wavevector<true>(g, idx, kk, ww));
        int j = -1;
        if (kmag >= ke0 && kmag < ke[nb]) j = find_bin(ke, nb, kmag, guess(kmag, ke0, kinv));
        double re = 0, im = 0;
        if (j >= 0) {
            CLoad<T>::get(in.p[j] + is.off(idx), re, im);
            if (deconv_pow) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    if (d >= g.ndim) continue;
                    const double sp = sinc_pow(ww[d], deconv_pow);
                    re /= sp;
                    im /= sp;
                }
            }
        }
        CLoad<T>::put(out + os.off(idx), re, im);
    }
}

#undef PMX_BLOCK_LOOP

// ---- pairsum ---------------------------------------------------------------------------------------------------------

constexpr int GWG = 1024;                     // threads of a pairsum workgroup: sixteen waves share a staged chunk
constexpr int GMAX_WG = 512;                  // workgroups at most: two per CU

struct BPairs {
    int64_t shape[3], s[3];                   // logical shape and common byte strides of the real blocks
    int64_t ncells, nchunks;
    int32_t nb, npairs;
};

__device__ __forceinline__ double lane_double(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// K cells per lane of a chunk of CH = 64 K cells, as in reduce_kernel: K / 2 runs of 128 cells, a wave on one of them
template <typename T, int K>
__global__ void __launch_bounds__(GWG) pairsum_kernel(BPairs g, BGIn f, BGOut o, const int32_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ pairs,
                                                      const double *__restrict__ weights)
{
    extern __shared__ __align__(16) double sm[];   // [nb][CH]
    __shared__ int32_t so[PMX_BISPEC_MAX_SHELLS + 1];
    constexpr int CH = 64 * K, R = K / 2, SSTEP = (GWG / 64) / R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = g.nb;
    const int run = wv % R, s0 = wv / R;
    const int64_t n12 = g.shape[1] * g.shape[2];

    // the entry ranges, forced into [0, npairs] and into order: whatever the list holds, no read leaves it
    for (int i = tid; i <= nb; i += GWG) so[i] = min(max(offsets[i], 0), g.npairs);

    for (int64_t chunk = blockIdx.x; chunk < g.nchunks; chunk += gridDim.x) {
        // stage: thread tid takes cell tid mod CH for every (GWG / CH)-th shell; one offset serves all of them
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
            for (int s = tid / CH; s < nb; s += GWG / CH) sm[s * CH + c] = in ? (double)*(const T *)(f.p[s] + off) : 0.0;
        }
        __syncthreads();

        // this lane's two cells of the wave's run, and where they live
        const int64_t n0 = chunk * CH + run * 128 + 2 * lane;
        const bool in0 = n0 < g.ncells, in1 = n0 + 1 < g.ncells;
        int64_t off0 = 0, off1 = 0;
        if (in0) {
            const int64_t i0 = n0 / n12, r = n0 - i0 * n12;
            const int64_t i1 = r / g.shape[2], i2 = r - i1 * g.shape[2];
            off0 = i0 * g.s[0] + i1 * g.s[1] + i2 * g.s[2];
        }
        if (in1) {
            const int64_t i0 = (n0 + 1) / n12, r = n0 + 1 - i0 * n12;
            const int64_t i1 = r / g.shape[2], i2 = r - i1 * g.shape[2];
            off1 = i0 * g.s[0] + i1 * g.s[1] + i2 * g.s[2];
        }
        const double2 *cells = (const double2 *)sm + run * 64 + lane;

        for (int s = s0; s < nb; s += SSTEP) {
            const int e0 = so[s], e1 = max(e0, so[s + 1]);
            double g0 = 0, g1 = 0;
            int pp = -1;
            double2 dp = make_double2(0, 0);
            for (int b = e0; b < e1; b += 64) {
                const int ne = min(64, e1 - b);
                int ep = -1, eq = -1;
                double ew = 0;
                if (lane < ne) {
                    ep = pairs[2 * (b + lane)];
                    eq = pairs[2 * (b + lane) + 1];
                    ew = weights[b + lane];
                }
                for (int e = 0; e < ne; e++) {
                    const int p = __builtin_amdgcn_readlane(ep, e), q = __builtin_amdgcn_readlane(eq, e);
                    // (a pair that names no shell reads nothing and adds nothing)
                    if ((unsigned)p >= (unsigned)nb || (unsigned)q >= (unsigned)nb) continue;
                    const double w = lane_double(ew, e);
                    if (p != pp) {
                        dp = cells[p * (CH / 2)];
                        pp = p;
                    }
                    const double2 dq = cells[q * (CH / 2)];
                    g0 += w * (dp.x * dq.x);
                    g1 += w * (dp.y * dq.y);
                }
            }
            char *dst = o.p[s];
            if (in0) *(T *)(dst + off0) = (T)g0;
            if (in1) *(T *)(dst + off1) = (T)g1;
        }
        __syncthreads();
    }
}

// cells per lane for nb shells: the staged chunk takes up to 64 KB of LDS (two workgroups per CU), as in pmx_bispec.hip
static int grad_cells_per_lane(int nb) { return nb <= 16 ? 8 : (nb <= 32 ? 4 : 2); }

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_bispec_pairsum(int32_t ndim, int32_t elsize, int32_t nb, const void *const *fields,
                                  void *const *outs, const int64_t *strides, const int64_t *shape, int32_t npairs,
                                  const int32_t *offsets, const int32_t *pairs, const double *weights, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && fields && outs && strides && shape && offsets, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nb >= 1 && npairs >= 0, PMX_EINVAL, "nb must be >= 1, npairs >= 0");
    PMX_REQUIRE(nb <= PMX_BISPEC_MAX_SHELLS, PMX_EUNSUPPORTED, "nb above PMX_BISPEC_MAX_SHELLS");
    PMX_REQUIRE(npairs <= 3 * PMX_BISPEC_MAX_TRIANGLES, PMX_EUNSUPPORTED, "npairs above 3 PMX_BISPEC_MAX_TRIANGLES");
    PMX_REQUIRE(npairs == 0 || (pairs && weights), PMX_EINVAL, "pairs and weights are needed for npairs > 0");
    BPairs g;
    BGIn f;
    BGOut o;
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
        o.p[s] = s < nb ? (char *)outs[s] : nullptr;
        PMX_REQUIRE(s >= nb || (f.p[s] && o.p[s]) || g.ncells == 0, PMX_EINVAL, "field or output pointer");
    }
    if (g.ncells == 0) return PMX_OK;
    const int K = grad_cells_per_lane(nb);
    g.nchunks = (g.ncells + 64 * K - 1) / (64 * K);
    g.nb = nb;
    g.npairs = npairs;
    const int nwg = (int)(g.nchunks < GMAX_WG ? g.nchunks : GMAX_WG);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        auto launch = [&](auto k) {
            constexpr int KC = decltype(k)::value;
            pairsum_kernel<T, KC><<<nwg, GWG, sizeof(double) * g.nb * 64 * KC, st>>>(g, f, o, offsets, pairs, weights);
        };
        if (K == 8) launch(int_c<8>{});
        else if (K == 4) launch(int_c<4>{});
        else launch(int_c<2>{});
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_bispec_shells_vjp(int32_t ndim, int32_t elsize, int32_t nb, int32_t deconv_pow,
                                     const void *const *in, const int64_t *in_strides, void *out,
                                     const int64_t *out_strides, const int64_t *shape, const int64_t *start,
                                     const int64_t *nmesh, const double *boxsize, const double *kedges, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && in && in_strides && out && out_strides && shape && start && nmesh &&
                boxsize && kedges, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nb >= 1, PMX_EINVAL, "nb must be >= 1");
    PMX_REQUIRE(nb <= PMX_BISPEC_MAX_SHELLS, PMX_EUNSUPPORTED, "nb above PMX_BISPEC_MAX_SHELLS");
    PMX_REQUIRE(deconv_pow >= 0, PMX_EINVAL, "deconv_pow must be >= 0");
    // memory order by decreasing stride of the output, axes of extent 1 slowest: the walk of pmx_bispec_shells
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides, AXES_UNIT_SLOWEST);
    for (int d = 0; d < 3; d++) PMX_REQUIRE(g.shape[d] >= 0 && g.nmesh[d] >= 1, PMX_EINVAL, "bad shape");
    BGIn f;
    for (int s = 0; s < PMX_BISPEC_MAX_SHELLS; s++) {
        f.p[s] = s < nb ? (const char *)in[s] : nullptr;
        PMX_REQUIRE(s >= nb || (f.p[s] && f.p[s] != out), PMX_EINVAL, "input pointer (null, or the output)");
    }
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        shells_vjp_kernel<T><<<grid, 256, 0, st>>>(g, nb, deconv_pow, f, is, (char *)out, os, kedges);
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
