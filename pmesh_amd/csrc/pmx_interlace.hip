// pmx_interlace.hip — the combine pass of interlaced painting (include/pmesh_amd.h: pmx_phase_combine;
// pmesh_amd/interlace.py): the spectrum of a mesh painted with a displaced transform is turned back by the phase of the
// displacement and averaged into the spectrum of the first mesh, with the window compensation of the result fused in.
//
// Replaces the ComplexField.apply loops a caller of the reference needs for it (nbodykit's interlaced painting: one
// pass for the phase over coordinate arrays, one for the sum, one for the compensation, with full-size complex
// temporaries).  One streaming kernel: one thread per mode in the memory order of `acc` (PMX_BLOCK_LOOP), two reads and
// one write per mode (one read when a == 0), the phase and the window recomputed from the index, no LDS.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

struct Shift {
    double twice[3];        // 2 * shift per axis, cells (0 beyond ndim)
};

// acc = ((ACC ? a * acc : 0) + b * exp(i theta) * in) / prod_d sinc(w_d / 2)^deconv_pow, theta = sum_d shift_d w_d
// (DECONV: deconv_pow != 0; without it the kernel holds no sin and about half the registers).
// theta / pi = sum_d 2 shift_d m_d / N_d with the signed mode number m_d: every term is reduced to [-1, 1] exactly
// (its own rounding, at most an ulp of the term before the reduction, is all it carries) and the sum goes to sincospi,
// so the phase is as accurate at |m| = 65536 as at m = 1: no product with a rounded pi, no reduction of a large angle.
template <typename T, bool ACC, bool DECONV>
__global__ void __launch_bounds__(256) phase_combine_kernel(Shift sh, double a, double b, int deconv_pow, BlockGeom g,
                                                            const char *in, BlockStr is, char *acc, BlockStr as)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double t = 0, comp = 1;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            if (d >= g.ndim) break;
            const int64_t gi = idx[d] + g.start[d], n = g.nmesh[d];
            const double m = (double)(gi >= n / 2 ? gi - n : gi);
            const double x = (sh.twice[d] * m) / (double)n;
            t += x - 2.0 * rint(0.5 * x);
            if (DECONV) comp *= sinc_pow(m * g.dw[d], deconv_pow);
        }
        double s, c;
        sincospi(t, &s, &c);
        double re, im;
        CLoad<T>::get(in + is.off(idx), re, im);
        double pr = b * (c * re - s * im), pi = b * (c * im + s * re);
        char *p = acc + as.off(idx);
        if (ACC) {
            double ar, ai;
            CLoad<T>::get(p, ar, ai);
            pr += a * ar;
            pi += a * ai;
        }
        if (DECONV) {
            pr /= comp;
            pi /= comp;
        }
        CLoad<T>::put(p, pr, pi);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

// the bytes [lo, hi) a strided block of complex elements of 2 * elsize bytes reaches
static void byte_span(const void *base, const BlockGeom &g, const BlockStr &s, int elsize, intptr_t &lo, intptr_t &hi)
{
    lo = hi = (intptr_t)base;
    for (int d = 0; d < 3; d++) {
        const int64_t reach = (g.shape[d] - 1) * s.s[d];
        if (reach < 0) lo += reach;
        else hi += reach;
    }
    hi += 2 * elsize;
}

extern "C" int pmx_phase_combine(int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides, void *acc,
                                 const int64_t *acc_strides, const int64_t *shape, const int64_t *start,
                                 const int64_t *nmesh, const double *shift, double a, double b, int32_t deconv_pow,
                                 void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    PMX_REQUIRE(in && in_strides && acc && acc_strides && shape && start && nmesh && shift, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(deconv_pow >= 0, PMX_EINVAL, "deconv_pow must not be negative");
    for (int d = 0; d < ndim; d++) PMX_REQUIRE(shape[d] >= 0 && nmesh[d] >= 1, PMX_EINVAL, "bad geometry");
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, nullptr, acc_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), as = make_str(ndim, acc_strides);
    intptr_t ilo, ihi, alo, ahi;
    byte_span(in, g, is, elsize, ilo, ihi);
    byte_span(acc, g, as, elsize, alo, ahi);
    PMX_REQUIRE(ihi <= alo || ahi <= ilo, PMX_EINVAL, "in and acc overlap");
    Shift sh;
    for (int d = 0; d < 3; d++) sh.twice[d] = d < ndim ? 2.0 * shift[d] : 0.0;
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(a != 0, [&](auto ac) {
            with_bool(deconv_pow != 0, [&](auto dc) {
                phase_combine_kernel<T, ac, dc><<<grid, 256, 0, st>>>(sh, a, b, deconv_pow, g, (const char *)in, is,
                                                                      (char *)acc, as);
            });
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
