// tf_align_icp_pyramid.h -- what tf_align_icp.hip asks of tf_align_icp_pyramid.hip: the levels of a call that runs the
// projective ICP with the handle's depth pyramid on (tf_align_icp_set_pyramid).  Host side only.
#pragma once

#include "tf_volume.h"

namespace tf {

// Level k = log2(stride) of a call, for every stride in its schedule (bit k of `used`): the image, the camera and the model
// maps the rows kernel is handed.  Level 0 is the caller's image at align_cam(v); its maps are AlignIcpState::maps, which
// the caller of icp_pyramid_enqueue fills in.
struct IcpLevels {
  AlignCam cam[4];
  const float* depth[4];
  float* vm[4];
  float* nm[4];
  uint32_t used;
};

bool icp_pyramid_on(const tf_volume* v);
// the camera of level k of `c` (include/tf_fusion.h has the derivation); exact in f32 for integer intrinsics
AlignCam icp_level_cam(const AlignCam& c, int k);
// What a call with the setting on is refused for: a stride of the first n_levels that is not 1, 2, 4 or 8 or does not
// divide the image's width and height.
int icp_pyramid_check(const tf_volume* v, const tf_align_params& geo, int n_levels);
// The level buffers grown to the camera, *out filled for the strides of the first n_levels of geo, and the one launch that
// builds every level image above 0 (none where the schedule is all stride 1).  d_cell != null: the launch returns at once
// where that cell holds no pose, as every launch of the device tracker does.
int icp_pyramid_enqueue(tf_volume* v, const float* d_depth, const tf_align_params& geo, int n_levels,
                        const tf_device_pose* d_cell, IcpLevels* out);
// tf_align_icp_residuals' maps of a level k >= 1: three level-sized maps (r, flags, assoc) for the rows launch to write ...
int icp_pyramid_residual_maps(tf_volume* v, int k, float** d_r, uint32_t** d_flags, int32_t** d_assoc);
// ... and their spread over the caller's full-size maps (any may be null): level pixel (X, Y) at (X << k, Y << k), 0, 0 and
// -1 everywhere else
int icp_pyramid_spread(tf_volume* v, int k, float* d_r, uint32_t* d_flags, int32_t* d_assoc);

}  // namespace tf
