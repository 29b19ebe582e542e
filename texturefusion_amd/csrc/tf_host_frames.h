// tf_host_frames.h -- what a handle owns for the per-frame host path (tf_integrate_frame_host, tf_host_*): a ring of
// pinned staging + device image slots with the H2D copies on a stream of their own, so that the copy of frame f + 1
// overlaps the kernels of frame f; the caller buffers registered for uploads in place; the frames staged but not yet
// launched.  The code is in tf_host_frames.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "tf_copy_pool.h"
#include "tf_mem.h"

struct tf_volume;

namespace tf {

struct HostFrames {
  // kHostDefer deferred frames + the one being staged + three whose kernels may still run (a frame's images are read by
  // its patch stage one launch behind its voxel update)
  static constexpr int kHostRing = 8;
  // frames tf_integrate_frame_host runs behind its caller: K-A of frame f - 4 shares its launch with the selection stages
  // of f - 3 and f - 2, like the streaming entry points; frames f - 1 and f are only being copied, so that no launch ever
  // has to wait for a copy in the stream
  static constexpr int kHostDefer = 4;

  struct HostSlot {
    PinMem h;                  // depth f32[npix] | rgba u8[4 npix]
    DevMem d;                  // depth | colour as uploaded (RGBA, or RGB + valid flags) | RGBA packed from an RGB upload
    hipEvent_t copied = nullptr;
    uint32_t free_when = 0;    // 0: free; else the progress stamp (tf_volume::h_progress) at which the last launch that reads d is through
  };
  HostSlot hslot[kHostRing];
  size_t hslot_pixels = 0;  // the camera all kHostRing slots fit and are laid out for; 0: the ring is not ready
  int hslot_next = 0;

  // caller buffers registered with tf_host_register (page-locked in place): host frames that lie inside one are uploaded
  // straight out of it -- no staging copy -- and the call returns when that upload is through
  struct HostRange { const uint8_t* p; size_t n; const uint8_t* locked; };  // locked: base of the process-wide page-locked range that covers it
  std::vector<HostRange> host_ranges;
  bool registered(const void* q, size_t n) const {  // [q, q + n) lies inside a registered range of this handle
    const uint8_t* b = static_cast<const uint8_t*>(q);
    for (const HostRange& r : host_ranges)
      if (b >= r.p && b + n <= r.p + r.n) return true;
    return false;
  }

  hipStream_t copy_stream = nullptr;
  hipStream_t copy_stream2 = nullptr;  // registered caller buffers: the colour image goes up next to the depth image (a second copy queue)
  hipEvent_t copy_join = nullptr;
  CopyPool* copy_pool = nullptr;  // helper threads of the staging copy (TF_COPY_THREADS, default 7)

  // frames staged but not integrated yet, oldest first
  struct Pending {
    const float* d = nullptr;
    const uint8_t* c = nullptr;
    float pose[12];
    float pinv[16];
    bool tex = false;
    int32_t fid = 0;
    int slot = 0;
    bool copied = false;  // its H2D copy is known to be complete, or the handle's stream has been told to wait for it
  };
  Pending pend[kHostDefer];
  int n_pend = 0;
  bool host_defer = true;            // tf_integrate_frame_host runs kHostDefer frames behind its caller (tf_host_frame_set_deferral)
  bool host_async = false;           // tf_host_frame_set_async: a call out of registered buffers returns before its upload is through
  hipEvent_t last_upload = nullptr;  // the newest frame's upload (tf_host_frame_fence waits for it)

  long host_waits = 0;  // copies a launch had to wait for in the stream (TF_HOST_TRACE prints it)
  double host_trace[6] = {0, 0, 0, 0, 0, 0};  // microseconds per phase of tf_integrate_frame_host, [5] = calls (tf_host_frame_times)

  // Gives back the events, the copy streams, the helper threads and the registered ranges, and prints the phase times
  // under TF_HOST_TRACE=1.  The slots' memory frees itself with the handle.
  void release();
};

bool host_defer_default();  // !(TF_HOST_DEFER=0 in the environment)
// brings the deferred frames onto the handle's stream, oldest first (TF_DEV_STREAM)
int flush_deferred(tf_volume* v);
// the last launch that reads a slot's device images is on the stream: the slot is free once that launch is through
void host_slot_release(tf_volume* v, int slot);

}  // namespace tf
