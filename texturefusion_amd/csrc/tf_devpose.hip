// tf_devpose.hip -- tracking and integrating a frame with the pose kept in device memory: KinectFusion's loop on the
// stream.  A pose lives in a tf_device_pose cell (include/tf_fusion.h); every launch that depends on a cell tests it on
// the device (tf_devpose.h: devpose_ok) and returns at once where it holds no pose, so a call is enqueued whole, up front,
// and nothing is read back.
//
//   k_pose_consts    one wave: the cell -> the handle's PoseConsts block: the Pose, the pose-dependent fields of
//                    make_select_consts' struct (tf_host_math.h, operation by operation: f32 multiplies and sequential
//                    adds, contraction off), the gate word.  The fields that depend on the resolution alone come from
//                    the host as an argument.  A second lane of the same launch writes the handle's PoseInverse block:
//                    devpose_inverse16 of the cell (tf_devpose.h) and the gate word again, for the patch stage.
//   k_track_finish   one lane: tf_track_frame's composition of its result (stage, pose), the acceptance test
//                    (tf_devpose.h: track_accepted, tf_relocalise's), the output cell
// and the twins that read a cell or the block, each next to the body it calls:
//   k_bbox_posed, k_select_posed (tf_kernels.hip)   K-B and K-C of the frame from the block; K-A never sees a pose
//   k_raycast_posed (tf_ray.hip)                    the model maps at the cell's pose
//   k_track_start (tf_align_icp.hip)                the projective stage starts from the cell
//   k_stage2_start (tf_align.hip)                   the SDF stage starts from the projective stage's result where it held
//   k_patch_posed (tf_atlas.hip)                    the patch stage of a frame projects with the PoseInverse block's matrix
//
// tf_track_frame_device:            raycast, projective stage, SDF stage, finish: 2 + 2 launches and 2 per evaluation
// tf_integrate_frame_posed_device:  consts, K-B, K-C, then the frame launch every integrated frame has (K-A)
// tf_integrate_frame_textured_posed_device: the same, the frame's mesher behind K-A, then the patch stage as a launch of
//                                   its own (k_patch_posed): it never rides on k_frame and is never pending across calls
// Not here: the posed patch stage as a role of k_frame, a textured form for a handle with untextured marks pending (the
// host cannot know the gate), a multi-rank form, a group or colour form of the device tracker, caching the tracked frame
// as a keyframe (the keyframe table's mirror lives on the host).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <string.h>

#include "tf_devpose.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

__global__ __launch_bounds__(64) void k_pose_consts(const tf_device_pose* __restrict__ cell, SelectConsts host,
                                                    PoseConsts* __restrict__ out, PoseInverse* __restrict__ inv) {
  const int lane = threadIdx.x;
  float p[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) p[i] = cell->pose[i];
  if (lane == 32) {  // the patch stage's matrix, next to lane 0's block
    float T[16];
    devpose_inverse16(p, T);
#pragma unroll
    for (int i = 0; i < 16; ++i) inv->T[i] = T[i];
    inv->gate = devpose_ok(cell) ? 1 : 0;
    inv->pad[0] = inv->pad[1] = inv->pad[2] = 0;
    return;
  }
  const float res = host.res;
  float rot[3][3];  // cameraPose.linear().transpose()
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) rot[i][j] = p[4 * j + i];
  if (lane < 8) {  // diffCentroidCoarse / diffCentroidRefine of corner k = x + 2 y + 4 z
    const float cur[3] = {(float)((lane & 1) * 8), (float)(((lane >> 1) & 1) * 8), (float)((lane >> 2) * 8)};
    const float half = res * 0.5f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float d = rot[a][0] * cur[0];
      d = d + rot[a][1] * cur[1];
      d = d + rot[a][2] * cur[2];
      out->sc.coarse[a][lane] = (d * res) * (float)host.step + half;
      out->sc.fine[a][lane] = (d * res) * 1.0f + half;
    }
  }
  if (lane != 0) return;
  SelectConsts& sc = out->sc;
  sc.res = res; sc.id_factor = host.id_factor; sc.step = host.step; sc.diag = host.diag; sc.diag_step = host.diag_step;
  sc.dtn_coarse = host.dtn_coarse; sc.dtn_fine = host.dtn_fine; sc.resDiag = host.resDiag; sc.plain = host.plain;
#pragma unroll
  for (int i = 0; i < 12; ++i) { sc.pose[i] = p[i]; out->P.p[i] = p[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) sc.rot[i][j] = rot[i][j];
    float s = rot[i][0] * p[3];  // rotation * cameraPose.translation(), sequential accumulation
    s = s + rot[i][1] * p[7];
    s = s + rot[i][2] * p[11];
    sc.tc[i] = s;
    sc.r0[i] = (rot[i][0] * 8.0f) * res;
    sc.r1[i] = (rot[i][1] * 8.0f) * res;
    sc.r2[i] = (rot[i][2] * 8.0f) * res;
  }
  out->gate = devpose_ok(cell) ? 1 : 0;
  out->pad[0] = out->pad[1] = out->pad[2] = 0;
}

struct FinishArgs {
  const tf_device_pose* start;
  tf_track_result* out;  // icp and sdf as the stages left them: a stage that did not run has written nothing
  tf_device_pose* pose_out;
  tf_track_accept acc;
  int has_accept;
};
__device__ __forceinline__ void put_not_run(tf_align_result* r) {  // {status -1, the rest 0}
  r->status = -1; r->evaluations = 0; r->n_sampled = 0; r->n_valid_first = 0; r->n_valid_last = 0;
  r->rms_first = 0.f; r->rms_last = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) r->pose[i] = 0.f;
}
__global__ __launch_bounds__(64) void k_track_finish(FinishArgs a) {
  if (threadIdx.x != 0) return;
  float start[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) start[i] = a.start->pose[i];  // (pose_out may be this cell: read before anything is written)
  const bool ok = devpose_ok(a.start);  // the ICP ran
  if (!ok) put_not_run(&a.out->icp);
  const int32_t s1 = a.out->icp.status;
  const bool held = s1 >= 0 && s1 <= TF_ALIGN_MAX_ITERS;  // the SDF stage ran
  if (!held) put_not_run(&a.out->sdf);
  const int32_t s2 = a.out->sdf.status;
  int32_t stage = 0;
  if (held) stage = (s2 >= 0 && s2 <= TF_ALIGN_MAX_ITERS) ? 2 : 1;
  float pose[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = stage == 2 ? a.out->sdf.pose[i] : (stage == 1 ? a.out->icp.pose[i] : start[i]);
  a.out->stage = stage;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.out->pose[i] = pose[i];
  const bool accepted = a.has_accept ? track_accepted(*a.out, a.acc.min_stage, a.acc.min_valid_fraction, a.acc.max_rms)
                                     : stage >= 1;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.pose_out->pose[i] = accepted ? pose[i] : start[i];
  a.pose_out->valid = accepted ? 1 : 0;
  a.pose_out->reserved[0] = a.pose_out->reserved[1] = a.pose_out->reserved[2] = 0;
}

// both blocks of the handle (first use: allocated)
int devpose_block(tf_volume* v, PoseConsts** pc) {
  int rc;
  if (!v->devpose && (rc = v->devpose.alloc(sizeof(PoseConsts)))) return rc;
  if (!v->devpose_inv && (rc = v->devpose_inv.alloc(sizeof(PoseInverse)))) return rc;
  *pc = v->devpose.as<PoseConsts>();
  return TF_OK;
}

void pose_consts_enqueue(tf_volume* v, const tf_device_pose* d_pose, PoseConsts* pc) {
  const float eye[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  const SelectConsts host = make_select_consts(eye, v->res);  // read for the resolution's fields; the pose's are the kernel's
  hipLaunchKernelGGL(k_pose_consts, dim3(1), dim3(64), 0, v->stream, d_pose, host, pc, v->devpose_inv.as<PoseInverse>());
}

bool partitioned(const tf_volume* v) {
  return v->dev.part_lo != INT32_MIN || v->dev.part_hi != INT32_MAX || v->comm.comm != nullptr;
}
bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int integrate_check(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const tf_device_pose* d_pose) {
  if (!v || !d_depth || !d_pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (partitioned(v)) { set_error("device pose: no form for a handle with a partition or a communicator"); return TF_ERR_INVALID; }
  if (!aligned_to(d_depth, 16) || !aligned_to(d_rgba, 4) || !aligned_to(d_pose, 16)) {
    set_error("device images and pose cells must be aligned (depth 16 B, rgba 4 B, cell 16 B)");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

int track_check_device(tf_volume* v, const float* d_depth, const tf_device_pose* d_start, const tf_align_icp_params* icp,
                       const tf_align_params* sdf, const tf_track_accept* accept, const tf_track_result* d_out,
                       const tf_device_pose* d_pose_out) {
  if (!v || !d_depth || !d_start || !icp || !sdf || !d_out || !d_pose_out) { set_error("null argument"); return TF_ERR_INVALID; }
  const float eye[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};  // the pose is checked on the device
  const int rc = track_check(v, d_depth, eye, icp, sdf);
  if (rc) return rc;
  if (v->ray_w > 0 && (v->ray_w != v->cam.W || v->ray_h != v->cam.H)) {
    set_error("device tracker: the raycast camera's size differs from tf_set_camera's");
    return TF_ERR_INVALID;
  }
  if (accept && (accept->min_stage < 1 || accept->min_stage > 2 ||
                 !(accept->min_valid_fraction >= 0.f && accept->min_valid_fraction <= 1.f) || !(accept->max_rms >= 0.f) ||
                 !isfinite(accept->max_rms))) {
    set_error("device tracker: need min_stage 1..2, min_valid_fraction in [0, 1], max_rms finite and >= 0");
    return TF_ERR_INVALID;
  }
  if (partitioned(v)) { set_error("device pose: no form for a handle with a partition or a communicator"); return TF_ERR_INVALID; }
  if (!aligned_to(d_start, 16) || !aligned_to(d_pose_out, 16) || !aligned_to(d_out, 4)) {
    set_error("device tracker: pose cells must be 16-byte aligned, the result 4-byte aligned");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

// every launch of the tracker: the projective stage from *d_start, the SDF stage from its result, the finish
int track_enqueue(tf_volume* v, const float* d_depth, const tf_device_pose* d_start, const tf_align_icp_params& icp,
                  const tf_align_params& sdf, const tf_track_accept* accept, tf_track_result* d_out,
                  tf_device_pose* d_pose_out) {
  const int32_t* d_status = nullptr;
  int rc = track_icp_posed(v, d_depth, d_start, icp, &d_out->icp, &d_status);
  if (rc || (rc = track_sdf_posed(v, d_depth, d_status, d_out->icp.pose, sdf, &d_out->sdf))) return rc;
  FinishArgs a{};
  a.start = d_start; a.out = d_out; a.pose_out = d_pose_out;
  if (accept) { a.acc = *accept; a.has_accept = 1; }
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(64), 0, v->stream, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// The frame's selection from *d_pose, then the frame launch of tf_integrate_frames_device(v, 1, ..): to enqueue_frames the
// frame is one whose selection a streaming call made ahead, so it goes on with K-A at once, carries a pending patch stage,
// stamps the progress word and advances the handle's counters exactly as a host-pose frame does.  K-A reads no pose.
// frame_id != NULL: the textured unit, tf_stream_frames_textured_device(v, 1, 0, ..)'s -- the frame's mesher behind K-A, then
// its patch stage as a launch of its own with the matrix k_pose_consts left in the handle's PoseInverse block.
int integrate_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const tf_device_pose* d_pose,
                      const int32_t* frame_id = nullptr) {
  PoseConsts* pc = nullptr;
  int rc = devpose_block(v, &pc);
  if (rc) return rc;
  if (v->n_primed) discard_primed(v);  // a stream that changed course
  pose_consts_enqueue(v, d_pose, pc);
  VolumeDev d = v->dev;
  d.sel = v->selbuf[(v->cur_sel + 1) % tf_volume::kSelSets];
  launch_bbox_posed(d, d_depth, v->cam, pc, v->stream);
  launch_select_posed(d, d_depth, v->cam, v->ig, pc, v->stream);
  TF_HIP(hipGetLastError());
  const float none[12] = {};
  v->primed[0].depth = d_depth;
  memcpy(v->primed[0].pose, none, sizeof(none));
  v->n_primed = 1;
  const TexturedArgs tex{nullptr, frame_id ? *frame_id : 0, v->devpose_inv.as<PoseInverse>()};
  if ((rc = enqueue_frames(v, 1, 0, &d_depth, d_rgba ? &d_rgba : nullptr, none, frame_id ? &tex : nullptr))) return rc;
  return bind_frame(v, d_depth, d_rgba);
}

// what the textured forms refuse on top of integrate_check: from the arguments ...
int textured_check(const uint8_t* d_rgba) {
  if (!d_rgba) { set_error("the textured flow needs a colour image per frame"); return TF_ERR_INVALID; }
  return TF_OK;
}
// ... and from the handle's state, once the frames and the patch stage it still owed are on the stream
int textured_state_check(const tf_volume* v) {
  if (v->atlas.phase1_on) {
    set_error("a texture stage is half done: call tf_texture_frame_device_phase(.., 2) first");
    return TF_ERR_INVALID;
  }
  if (v->clear_floor < v->epoch) {
    set_error("device pose: frames integrated without texturing are still waiting for a mesher, and a cell that holds no "
              "pose would clear their marks without patches: texture them first (tf_texture_frame_device)");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

}  // namespace

void devpose_release(tf_volume* v) {
  v->devpose = DevMem{};
  v->devpose_inv = DevMem{};
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_track_accept_default(tf_track_accept* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_track_accept a{};
  a.min_stage = 2;
  a.min_valid_fraction = 0.5f;
  a.max_rms = 0.01f;
  *out = a;
  return TF_OK;
}

int tf_track_frame_device(tf_volume* v, const float* d_depth, const tf_device_pose* d_start, const tf_align_icp_params* icp,
                          const tf_align_params* sdf, const tf_track_accept* accept, tf_track_result* d_out,
                          tf_device_pose* d_pose_out) {
  const int rc = track_check_device(v, d_depth, d_start, icp, sdf, accept, d_out, d_pose_out);
  if (rc) return rc;
  TF_DEV_READER(v);
  return track_enqueue(v, d_depth, d_start, *icp, *sdf, accept, d_out, d_pose_out);
}

int tf_integrate_frame_posed_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const tf_device_pose* d_pose) {
  const int rc = integrate_check(v, d_depth, d_rgba, d_pose);
  if (rc) return rc;
  TF_DEV_STREAM(v);
  return integrate_enqueue(v, d_depth, d_rgba, d_pose);
}

int tf_track_integrate_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const tf_device_pose* d_start,
                              const tf_align_icp_params* icp, const tf_align_params* sdf, const tf_track_accept* accept,
                              tf_track_result* d_out, tf_device_pose* d_pose_out) {
  int rc = track_check_device(v, d_depth, d_start, icp, sdf, accept, d_out, d_pose_out);
  if (rc || (rc = integrate_check(v, d_depth, d_rgba, d_pose_out))) return rc;
  TF_DEV(v);
  if ((rc = track_enqueue(v, d_depth, d_start, *icp, *sdf, accept, d_out, d_pose_out))) return rc;
  return integrate_enqueue(v, d_depth, d_rgba, d_pose_out);
}

int tf_integrate_frame_textured_posed_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                             const tf_device_pose* d_pose, int32_t frame_id) {
  int rc = integrate_check(v, d_depth, d_rgba, d_pose);
  if (rc || (rc = textured_check(d_rgba))) return rc;
  TF_DEV_STREAM(v);  // (a patch stage an earlier streaming call left pending rides on this frame's launch, as on any frame's)
  if ((rc = textured_state_check(v))) return rc;
  return integrate_enqueue(v, d_depth, d_rgba, d_pose, &frame_id);
}

int tf_track_texture_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const tf_device_pose* d_start,
                            const tf_align_icp_params* icp, const tf_align_params* sdf, const tf_track_accept* accept,
                            tf_track_result* d_out, tf_device_pose* d_pose_out, int32_t frame_id) {
  int rc = track_check_device(v, d_depth, d_start, icp, sdf, accept, d_out, d_pose_out);
  if (rc || (rc = integrate_check(v, d_depth, d_rgba, d_pose_out)) || (rc = textured_check(d_rgba))) return rc;
  TF_DEV(v);
  if ((rc = textured_state_check(v))) return rc;
  if ((rc = track_enqueue(v, d_depth, d_start, *icp, *sdf, accept, d_out, d_pose_out))) return rc;
  return integrate_enqueue(v, d_depth, d_rgba, d_pose_out, &frame_id);
}

int tf_pose_inverse_download(tf_volume* v, const tf_device_pose* d_pose, void* out, size_t bytes) {
  if (!v || !d_pose || !out) { set_error("null argument"); return TF_ERR_INVALID; }
  if (bytes > sizeof(PoseInverse) || !aligned_to(d_pose, 16)) {
    set_error("pose inverse: at most 80 bytes, from a 16-byte aligned cell");
    return TF_ERR_INVALID;
  }
  TF_DEV_READER(v);
  PoseConsts* pc = nullptr;
  const int rc = devpose_block(v, &pc);
  if (rc) return rc;
  pose_consts_enqueue(v, d_pose, pc);
  TF_HIP(hipGetLastError());
  TF_HIP(hipMemcpyAsync(out, v->devpose_inv.p, bytes, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  return TF_OK;
}

int tf_pose_consts_download(tf_volume* v, const tf_device_pose* d_pose, void* out, size_t bytes) {
  if (!v || !d_pose || !out) { set_error("null argument"); return TF_ERR_INVALID; }
  if (bytes > sizeof(PoseConsts) || !aligned_to(d_pose, 16)) {
    set_error("pose consts: at most 424 bytes, from a 16-byte aligned cell");
    return TF_ERR_INVALID;
  }
  TF_DEV_READER(v);
  PoseConsts* pc = nullptr;
  const int rc = devpose_block(v, &pc);
  if (rc) return rc;
  pose_consts_enqueue(v, d_pose, pc);
  TF_HIP(hipGetLastError());
  TF_HIP(hipMemcpyAsync(out, pc, bytes, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  return TF_OK;
}

}  // extern "C"
