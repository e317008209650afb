"""calibration_amd — MI355X-native bundle-adjustment engine (libcalibba) and its host-side mirror
of VitalyVorobyev/calibration's ``calib::estimation_optim`` refinement API.

The compute path is the HIP library behind ``include/calibba.h``; this package only loads it
(ctypes) and flattens host containers into the SoA buffers the C ABI takes.  There is no CPU
fallback: every compute entry point raises if the HIP library or a GPU is missing.
"""
from .capi import (  # noqa: F401
    CbaError,
    CbaOptions,
    CbaReprojProblem,
    CbaSummary,
    load_library,
    library_path,
)
from .optim import (  # noqa: F401
    BundleObservation,
    BundleOptions,
    ExtrinsicOptions,
    IntrinsicsOptimOptions,
    OptimOptions,
    ReprojHandle,
    optimize_bundle,
    optimize_extrinsics,
    optimize_handeye,
    optimize_intrinsics,
    optimize_planar_pose,
    optimize_planar_pose_batch,
    PlanarPoseOptions,
)
from .linescan import (  # noqa: F401
    LaserProfiles,
    LaserScanner,
    LaserScanOptions,
    laser_points,
    LinescanCalibrationFacade,
    LineScanPlaneFitOptions,
    LineScanView,
    RansacOptions,
    calibrate_laser_plane,
    fit_plane_ransac,
    fit_plane_svd,
    invert_brown_conrady,
    plane_rms,
    points_from_view,
)
from .linear import (  # noqa: F401
    HomographyResult,
    IntrinsicsEstimOptions,
    IntrinsicsEstimateResult,
    ViewEstimateData,
    calibrate_planar_intrinsics,
    estimate_homography,
    estimate_homography_batch,
    estimate_intrinsics,
    pose_from_homography,
    sanitize_intrinsics,
    zhang_intrinsics_from_hs,
)
from .rig import (  # noqa: F401
    ExtrinsicPoses,
    RigCalibrationResult,
    calibrate_rig,
    estimate_extrinsic_dlt,
)

from .handeye_rig import (  # noqa: F401
    BundleRigResult,
    BundleSeed,
    HandeyeRigResult,
    calibrate_bundle_rig,
    calibrate_handeye_rig,
    estimate_bundle_seed,
    estimate_bundle_seed_blocks,
)
from .distortion import (  # noqa: F401
    DistortionWithResiduals,
    DualDistortionWithResiduals,
    PinholeBrownConrady,
    estimate_intrinsics_linear,
    estimate_intrinsics_linear_batch,
    estimate_intrinsics_linear_iterative,
    estimate_intrinsics_linear_iterative_batch,
    fit_distortion,
    fit_distortion_batch,
    fit_distortion_dual,
    fit_distortion_full,
)
from .camera import (  # noqa: F401
    UndistortMap,
    distort,
    project,
    undistort,
    unproject,
)
from .stereo import (  # noqa: F401
    DisparityFilter,
    DisparityFilterOptions,
    SgmMatcher,
    SgmOptions,
    StereoGeometry,
    StereoMatcher,
    StereoMatchOptions,
    StereoRectification,
    StereoResult,
    rectify,
    rectify_maps,
    stereo_points,
)
from .detect import (  # noqa: F401
    BlobDetector,
    BlobOptions,
    BlobResult,
    BoardDetection,
    CornerDetector,
    CornerOptions,
    CornerResult,
    circle_centre_bias,
    detect_chessboard,
    detect_circle_grid,
    order_chessboard,
    order_circle_grid,
)
from .triangulate import (  # noqa: F401
    TriangulateOptions,
    TriangulationResult,
    triangulate,
)
from .registration import (  # noqa: F401
    AlignEdge,
    AlignResult,
    CloudIndex,
    CloudSet,
    IcpOptions,
    IcpResult,
    align,
    edges_from_overlaps,
    point_normals,
    register,
)
from .fusion import (  # noqa: F401
    Mesh,
    RayCast,
    RayCastOptions,
    TsdfOptions,
    TsdfVolume,
    depth_from_xyz,
    fuse,
    read_ply,
    rgba_maps,
    track,
    write_ply,
)
from .structured_light import (  # noqa: F401
    Decoded,
    StructuredLightDecoder,
    StructuredLightOptions,
    image_count,
    patterns,
    projector_corners,
)
from .diagnostics import (  # noqa: F401
    ResidualStats,
    RobustOptions,
    RobustResult,
    build_planar_intrinsics_report,
    bundle_view_errors,
    compute_global_rms,
    extrinsic_view_errors,
    refine_with_outlier_rejection,
    subset_problem,
    view_errors,
)

__version__ = "0.1.0"
