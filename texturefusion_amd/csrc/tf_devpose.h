// tf_devpose.h -- a pose kept in device memory (tf_device_pose, include/tf_fusion.h) as the kernels see it: the test every
// launch that depends on a pose cell makes, and the block k_pose_consts (tf_devpose.hip) derives from a cell for the
// selection launches, with the pose's rigid inverse in a block of its own for the patch stage.  The kernels that read any of
// them are the thin twins next to the bodies they call: k_bbox_posed and k_select_posed (tf_kernels.hip), k_raycast_posed
// (tf_ray.hip), the trackers' start kernels (tf_align.hip, tf_align_icp.hip), k_patch_posed (tf_atlas.hip).
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

// What the patch stage needs of a frame's pose, in a second block the handle owns (tf_volume::devpose_inv): T is
// devpose_inverse16 of the cell, KfDev::T of a frame textured from a device pose (k_patch_posed, tf_atlas.hip).  gate == 0:
// the cell held no pose, T is the same arithmetic on whatever the cell stores, and nobody reads it for work.
struct PoseInverse {
  float T[16];
  int32_t gate;
  int32_t pad[3];
};
static_assert(sizeof(PoseInverse) == 80, "PoseInverse is what tf_pose_inverse_download hands out");

// The rigid inverse [R^T | -R^T t; 0 0 0 1] of a row-major 3 x 4 pose, row-major 4 x 4: the definition of the matrix a frame
// tracked on the device is textured with, on the host and on the device.  The rotation is copied; a translation entry is
// the f32 of a sum of three f64 products of f32 values -- each exact -- added left to right, so the order of the two
// additions is all there is to restate (tests/pose_inverse_ref.py), whether or not the compiler fuses them.  It is
// rigid_inverse (tf_reloc.hip) run the other way.
__host__ __device__ inline void devpose_inverse16(const float pose[12], float T[16]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) T[4 * r + c] = pose[4 * c + r];
    const double t = ((double)pose[r] * (double)pose[3] + (double)pose[4 + r] * (double)pose[7]) +
                     (double)pose[8 + r] * (double)pose[11];
    T[4 * r + 3] = (float)-t;
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

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
