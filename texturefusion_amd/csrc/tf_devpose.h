// tf_devpose.h -- a pose kept in device memory (tf_device_pose, include/tf_fusion.h) as the kernels see it: the test every
// launch that depends on a pose cell makes, and the block k_pose_consts (tf_devpose.hip) derives from a cell for the
// selection launches.  The kernels that read either are the thin twins next to the bodies they call: k_bbox_posed and
// k_select_posed (tf_kernels.hip), k_raycast_posed (tf_ray.hip), the trackers' start kernels (tf_align.hip,
// tf_align_icp.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/tf_fusion.h"
#include "tf_device.h"
#include "tf_host_math.h"

namespace tf {

// What a frame's selection needs of its pose, in a block the handle owns (tf_volume::devpose).  sc is make_select_consts'
// struct: the fields that depend on the resolution alone come from the host through k_pose_consts' arguments, the rest is
// computed by that kernel from the cell.  gate == 0: the cell held no pose, and every launch that reads the block returns
// at once (sc and P then hold the cell's numbers all the same: nothing reads them).
struct PoseConsts {
  SelectConsts sc;
  Pose P;
  int32_t gate;
  int32_t pad[3];
};
static_assert(sizeof(PoseConsts) == 424, "PoseConsts is what tf_pose_consts_download hands out");
static_assert(sizeof(tf_device_pose) == 64, "tf_device_pose");

// Is a tracker's result good enough: tf_relocalise's test of a try on the host, and tf_track_frame_device's of its result
// on the device -- one text, every operation f32 and rounded on its own.  The figures are those of the stage that gave
// the pose.
__host__ __device__ inline bool track_accepted(const tf_track_result& t, int32_t min_stage, float min_valid_fraction,
                                               float max_rms) {
  const tf_align_result& a = t.stage == 2 ? t.sdf : t.icp;
  return t.stage >= min_stage && a.n_sampled > 0 && (float)a.n_valid_last >= min_valid_fraction * (float)a.n_sampled &&
         a.rms_last <= max_rms;
}

// does the cell hold a pose: valid set and every entry finite
__device__ __forceinline__ bool devpose_ok(const tf_device_pose* c) {
  bool ok = c->valid != 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && isfinite(c->pose[i]);
  return ok;
}

// the same asked by a whole wave that has loaded the cell's entries one per lane (entry: pose[lane] for lane < 12, any
// entry elsewhere)
__device__ __forceinline__ bool devpose_ok_wave(const tf_device_pose* c, float entry) {
  return c->valid != 0 && __all(isfinite(entry) ? 1 : 0);
}

}  // namespace tf
