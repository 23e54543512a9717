"""pmesh_amd — the particle-mesh cycle of MP-Gadget/pmesh on AMD MI355X (gfx950).

    from pmesh_amd.pm import ParticleMesh, RealField, ComplexField
    from pmesh_amd.window import ResampleWindow, Affine, CIC, TSC, PCS
    from pmesh_amd.domain import GridND, Layout
    from pmesh_amd.transfer import Transfer, Tabulated
    from pmesh_amd.power import power_spectrum     # binned P(k), P(k, mu), multipoles
    from pmesh_amd.bispectrum import bispectrum    # binned B(k1, k2, k3) over closed triangle bins, counts, Q
    from pmesh_amd.bispectrum import bispectrum_vjp, bispectrum_jvp   # and its gradients
    from pmesh_amd.survey import survey_multipoles, multipole_field   # P_0,2,4 with a local line of sight (Yamamoto)
    from pmesh_amd.interlace import paint_interlaced, interlaced_field   # alias-cancelling spectra (interlacing)
    from pmesh_amd.correlation import correlation_function, correlation_field, bin_real   # xi(r), xi(r, mu), xi_l(r)
    from pmesh_amd.correlation import correlation_function_vjp, correlation_function_jvp   # and their gradients
    from pmesh_amd.mock import poisson_sample, lognormal_catalog   # particles Poisson-sampled from a field; lognormal mocks
    from pmesh_amd.fof import fof, fof_catalog                     # friends-of-friends groups and a halo catalogue
    from pmesh_amd.paircount import pair_counts, pair_correlation   # binned pair counts and xi(r), xi(r, mu), xi(rp, pi)
    from pmesh_amd.surveypairs import survey_pair_counts, survey_correlation   # xi(s, mu), wp(rp), w(theta) of a survey: pairwise line of sight
    from pmesh_amd.surveypairs import to_poles, to_wp, sky_to_cartesian   # and what goes with them
    from pmesh_amd.threept import threept_multipoles, threept_correlation   # three-point multipoles zeta_l(r1, r2) of particles
    from pmesh_amd.shortrange import short_range_force              # the short-range pair force of a TreePM / P3M split
    from pmesh_amd.knn import knn, knn_density, knn_cdf             # k-nearest-neighbour distances, densities and the kNN-CDF
    from pmesh_amd.profiles import radial_profiles, so_masses      # per-centre radial profiles, Sigma(R) and spherical-overdensity masses
    from pmesh_amd.pairvel import pairwise_velocities, pairwise_los   # pairwise velocities v12(r), their dispersions, v_los(rp, pi); the kSZ pairwise estimator
    from pmesh_amd.pairlabels import pair_counts_jackknife, pair_correlation_jackknife   # delete-one jackknife counts, xi and its covariance in one walk over the pairs
    from pmesh_amd.pairlabels import survey_pair_counts_jackknife, survey_correlation_jackknife   # the same about an observer
    from pmesh_amd.pairlabels import pair_counts_split, pair_correlation_split, box_regions   # the one-halo / two-halo split; sub-box labels
    from pmesh_amd.alignments import alignment_counts, projected_alignment_counts   # intrinsic alignments: omega(r), eta(r), w_g+(rp), w_++(rp)
    from pmesh_amd.alignments import ellipticity_from_orientation   # the projected spin-2 ellipticity of a 3-d axis
    from pmesh_amd.moments import radial_moments, halo_shapes, ellipticity_from_shapes   # per-centre moment sums: halo shapes, spins and dispersions
    from pmesh_amd.lpt import lpt, lpt1, lpt2source  # 1LPT / 2LPT displacements of initial conditions
    from pmesh_amd.lpt import lpt_vjp, lpt_jvp, lpt2source_vjp, lpt2source_jvp   # and their gradients

Host code is Python; all arithmetic is in libpmesh_amd.so (hand-written HIP
kernels + rocFFT behind the C ABI of include/pmesh_amd.h).  Importing the
package does not touch the GPU; the first operation does, and raises if the
library or the device is missing — there is no CPU fallback.
"""
__version__ = '0.1.0'
