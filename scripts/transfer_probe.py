"""Times transfer_kernel (csrc/pmx_transfer.hip) alone: pmx_apply_transfer on an N x N x (N/2+1) spectrum, out of place.

For f8 and f4 and the forms
    dx1, potential              the SIMPLE kernel (the transfers of the PM cycle)
    finite4, deconv2, gauss     the general kernel (finite-difference gradient, window deconvolution, Gaussian)
prints one JSON line per case: the median and the minimum of --reps launches (HIP events), in ms.

    python scripts/transfer_probe.py [--mesh 512] [--reps 30]
A/B of two builds: run it once per library (PMESH_AMD_LIBRARY), each in a process of its own, alternating.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import _abi, backend  # noqa: E402

FORMS = (('dx1', dict(laplace_pow=-1, grad_dir=2, grad_kind=0)), ('potential', dict(amplitude=-1.0, laplace_pow=-1)),
         ('finite4', dict(laplace_pow=-1, grad_dir=0, grad_kind=1)), ('deconv2', dict(deconv_pow=2)),
         ('gauss', dict(gauss_r=3.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    N = args.mesh
    be = backend.get()
    for dt, rdt in (('f8', torch.float64), ('f4', torch.float32)):
        a = torch.view_as_complex(torch.randn((N, N, N // 2 + 1, 2), device=be.device, dtype=rdt))
        out = torch.empty_like(a)
        es = a.element_size()
        for form, kw in FORMS:
            t = _abi.Transfer()
            t.amplitude, t.grad_dir = 1.0, -1
            for k, v in kw.items():
                setattr(t, k, v)

            def run():
                be.call('apply_transfer', C.byref(t), 3, es // 2, a.data_ptr(), _abi.i64arr([s * es for s in a.stride()], 3),
                        out.data_ptr(), _abi.i64arr([s * es for s in out.stride()], 3), _abi.i64arr(a.shape, 3),
                        _abi.i64arr((0, 0, 0), 3), _abi.i64arr((N, N, N), 3), _abi.f64arr((1000.,) * 3, 3), be.stream())
            run()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            print(json.dumps({'probe': 'transfer', 'mesh': N, 'dtype': dt, 'case': form,
                              'kernel_ms': round(float(numpy.median(ts)), 4), 'min_ms': round(min(ts), 4)}), flush=True)
        del a, out


if __name__ == '__main__':
    main()
