// tf_align_exposure.h -- how the two photometric aligners hand a call to tf_align_exposure.hip where tf_align_set_exposure is
// on.  The aligner keeps what is its own (its state block with control words, poses and log, its checks, its staging, the
// colour ICP its model maps); the launches that read or estimate the exposure pair are the other file's.
#pragma once

#include "tf_align_icp_rows.h"
#include "tf_align_rows.h"
#include "tf_volume.h"

namespace tf {

// the calling aligner's own state: pose_f and pose_r hold 12 floats, with a model pose 24
struct ExposureOwn {
  AlignCtl* ctl;
  double* pose_d;
  float* pose_f;
  float* pose_r;
  tf_align_color_iter* log;
};

bool exposure_on(const tf_volume* v);
// aligner `which` (0: tf_align_color.hip, 1: tf_align_icp_color.hip) enqueues a call with the setting off: nothing is
// launched, the exposure log of that aligner is empty from now on
void exposure_not_run(tf_volume* v, int which);
// Every launch of one alignment but the colour ICP's model maps: begin (the start pair read from the cell), then (rows,
// solve) per step and once more to close.  `ra`: the rows launch's arguments but level, pose, state and sums.
int exposure_sdf_enqueue(tf_volume* v, const ExposureOwn& o, const AlignPose& start, CAlignRowsArgs ra, const tf_align_params& geo,
                         double l2, tf_align_color_result* d_result);
int exposure_proj_enqueue(tf_volume* v, const ExposureOwn& o, const float* pose, const float* model_pose, CicpRowsArgs ra,
                          const tf_align_params& geo, double l2, tf_align_color_result* d_result);
// The residual maps at the cell's current pair: begin (poses and pair alone) and one rows launch with `ra` as it is but its pose.
int exposure_sdf_residuals(tf_volume* v, const ExposureOwn& o, const AlignPose& pose, CAlignRowsArgs ra, uint32_t n_rows);
int exposure_proj_residuals(tf_volume* v, const ExposureOwn& o, const float* pose, const float* model_pose, CicpRowsArgs ra,
                            uint32_t n_rows);
// tf_track_frame_color around its stages.  1: the first stage is about to run (its estimate goes to the cell whatever carry
// says); 0: it has been enqueued; 2: the second stage has run (with carry off the cell gets the start pair back).
int exposure_track_stage(tf_volume* v, int stage);
void align_exposure_release(tf_volume* v);

}  // namespace tf
