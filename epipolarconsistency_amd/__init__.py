"""epipolarconsistency_amd -- MI355X-native epipolar-consistency hot path.

Radon intermediates + all-pairs ECC behind the reference's RadonIntermediate /
MetricRadonIntermediate interface (aaichert/EpipolarConsistency).  The compute lives in
libecc_hip.so (hand-written HIP for gfx950, C ABI in include/ecc_hip.h); this package is the thin
host mirror.  Importing the package does not load the library; the first API call does and fails
loudly if it has not been built.
"""
from ._lib import (EccError, FILTER_DERIVATIVE, FILTER_NONE, FILTER_RAMP, LOSS_GEMAN_MCCLURE, LOSS_HUBER, LOSS_TRUNCATED, POST_IDENTITY,
                   POST_LOGARITHM, POST_SQUARE_ROOT)
from . import geometry
from .api import (Context, Group, GroupMetricRadonIntermediate, MetricDirect, MetricRadonIntermediate, pair_shard, pair_shards_balanced, PreProccess, RadonIntermediate, direct_pose_pairs, get_ij, host_object_radius, host_pinvT,
                  host_source_position, pack_projection_matrices, slab_floats, estimateAngularRange, estimateAngularStep,
                  estimateIsoCenter, estimateObjectRadius, gram_minimizer, gram_value, line_weights, line_weights_device, line_weights_from_lengths,
                  minimize_view_coefficients, refine_line_weights, refine_variances, robust_scale, histogram_quantile, sample_robust_scale, variance_floor, variance_intermediates, variance_robust_scale, view_hessian_minimizer, view_hessian_value, weighted_robust_scale)

__all__ = ["Context", "Group", "GroupMetricRadonIntermediate", "pair_shard", "pair_shards_balanced", "MetricDirect", "PreProccess", "RadonIntermediate", "MetricRadonIntermediate", "EccError", "direct_pose_pairs", "get_ij", "slab_floats", "pack_projection_matrices", "host_pinvT",
           "host_source_position", "host_object_radius", "FILTER_DERIVATIVE", "FILTER_RAMP", "FILTER_NONE",
           "POST_IDENTITY", "POST_SQUARE_ROOT", "POST_LOGARITHM", "estimateAngularRange", "estimateAngularStep",
           "estimateIsoCenter", "estimateObjectRadius", "gram_minimizer", "gram_value", "minimize_view_coefficients",
           "view_hessian_minimizer", "view_hessian_value", "line_weights", "line_weights_from_lengths", "line_weights_device", "LOSS_HUBER", "LOSS_TRUNCATED",
           "LOSS_GEMAN_MCCLURE", "robust_scale", "weighted_robust_scale", "refine_line_weights", "refine_variances", "variance_floor", "variance_intermediates", "variance_robust_scale", "histogram_quantile", "sample_robust_scale"]
