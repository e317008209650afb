// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the extrinsics check's stand-in declarations (ext_min.h) plus the one record
// include/calibba_handeye_rig.hpp reads, calib::BundleObservation with the reference's member names (estimation/optim/bundle.h).
// It pins nothing; in the reference's tree the header is compiled against the real headers.
#pragma once
#include <cmath>

#include "../../extrinsics_adapter_check/stand_ins/ext_min.h"

namespace calib {
struct BundleObservation final {
    PlanarView view;
    Eigen::Isometry3d b_se3_g;
    size_t camera_index = 0;
};
}  // namespace calib
