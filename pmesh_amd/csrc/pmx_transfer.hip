// pmx_transfer.hip — apply-transfer on the complex field, one thread per mode.
//
// Replaces the Python slab loop of Field.apply (pmesh/pm.py:617-648) for the
// transfer functions used in the PM cycle (examples/nbody.py:154-181,
// pmesh/transfer.py:69-112,232-240, window compensation window.py:65-80).
// Coordinates follow _init_o_coords (pm.py:1200-1226): w = 2 pi/N (i - N[i>=N/2]),
// k = w N / L, Nyquist negative.  HBM-bound: one complex read + one complex
// write per mode; the k-vectors are recomputed from the index (no coordinate
// arrays are read).
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

// One thread per mode in memory order (PMX_BLOCK_LOOP), k in the transfer kernels' own sequence w * (N / L) (k_scaled).
// SIMPLE: no Gaussian, no deconvolution, spectral or no gradient — the transfers of the PM
// cycle proper (dx1, potential): no transcendental code, few registers, high occupancy.
template <typename T, bool SIMPLE>
__global__ void __launch_bounds__(256) transfer_kernel(pmx_transfer t, BlockGeom g, const char *in, BlockStr is, char *out,
                                                       BlockStr os)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3], ww[3];
        const double k2 = wavevector(g, idx, kk, ww);
        double re = t.amplitude, im = 0;
        if (t.laplace_pow) {
            double qq = (k2 == 0) ? 1.0 : k2;
            if (t.laplace_pow == -1) re *= 1.0 / qq;
            else if (t.laplace_pow == 1) re *= qq;
            else if (!SIMPLE) re *= pow(qq, (double)t.laplace_pow);
        }
        if (!SIMPLE && t.gauss_r != 0) re *= exp(-0.5 * k2 * t.gauss_r * t.gauss_r);
        if (!SIMPLE && t.deconv_pow) {
            for (int d = 0; d < g.ndim; d++) re /= sinc_pow(ww[d], t.deconv_pow);
        }
        if (t.grad_dir >= 0) {
            int d = t.grad_dir;
            double D;
            if (SIMPLE || t.grad_kind == 0) D = kk[d];
            else {
                double C = g.boxsize[d] / g.nmesh[d];
                double w = kk[d] * C;
                D = 1.0 / C * 1 / 6.0 * (8 * sin(w) - sin(2 * w));
            }
            im = re * D;
            re = 0;
        }
        double ar, ai;
        CLoad<T>::get(in + is.off(idx), ar, ai);
        CLoad<T>::put(out + os.off(idx), re * ar - im * ai, re * ai + im * ar);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_apply_transfer(const pmx_transfer *t, int32_t ndim, int32_t elsize,
                                  const void *in, const int64_t *in_strides, void *out,
                                  const int64_t *out_strides, const int64_t *shape,
                                  const int64_t *start, const int64_t *nmesh,
                                  const double *boxsize, void *stream)
{
    PMX_REQUIRE(t && ndim >= 1 && ndim <= 3, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(t->grad_dir < ndim, PMX_EINVAL, "grad_dir out of range");
    // axes by decreasing output stride: consecutive threads touch consecutive memory whatever the (transposed) layout
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    const bool simple = t->gauss_r == 0 && t->deconv_pow == 0 && (t->grad_dir < 0 || t->grad_kind == 0) &&
                        t->laplace_pow >= -1 && t->laplace_pow <= 1;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(simple, [&](auto sm) {
            transfer_kernel<T, sm><<<grid, 256, 0, st>>>(*t, g, (const char *)in, is, (char *)out, os);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
