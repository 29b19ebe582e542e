// tf_host_frames.cpp -- the per-frame host path: tf_integrate_frame_host / _rgb and the tf_host_* entry points over
// tf_volume::hf (tf_host_frames.h).  Host code only; the launches themselves are enqueue_frames' (tf_capi.cpp).
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <thread>

#include "tf_locked_ranges.h"
#include "tf_volume.h"

namespace tf {

// Page-locking is a property of the PROCESS: two handles (two volumes on one GPU, or a volume per GPU) may be fed from the
// same caller buffers.  The ranges the library locked are counted here; the pages are locked by the first handle that
// registers a range and released by the last that lets go of it.
static std::mutex g_locked_mu;
static LockedRanges g_locked;
static int host_range_release(const uint8_t* p) {
  std::lock_guard<std::mutex> lk(g_locked_mu);
  if (g_locked.release(p)) TF_HIP(hipHostUnregister(const_cast<uint8_t*>(p)));
  return TF_OK;
}

bool host_defer_default() {
  static const bool on = !(getenv("TF_HOST_DEFER") && !atoi(getenv("TF_HOST_DEFER")));
  return on;
}
// TF_HOST_POLL_SLEEP_US > 0: the waits below sleep between polls instead of spinning -- several ranks under one CPU quota
static int poll_sleep_us() {
  static const int us = getenv("TF_HOST_POLL_SLEEP_US") ? atoi(getenv("TF_HOST_POLL_SLEEP_US")) : 0;
  return us;
}

void HostFrames::release() {
  for (const HostRange& r : host_ranges) (void)host_range_release(r.locked);
  for (HostSlot& s : hslot)
    if (s.copied) hipEventDestroy(s.copied);
  if (host_trace[5] > 0 && getenv("TF_HOST_TRACE") && atoi(getenv("TF_HOST_TRACE")))
    fprintf(stderr, "tf host frames: %.0f calls; per call us: wait kernels %.1f, wait upload %.1f, staging copy %.1f, "
                    "upload enqueue %.1f, launches %.1f; copies a launch waited for in the stream: %ld\n", host_trace[5],
            host_trace[0] / host_trace[5], host_trace[1] / host_trace[5], host_trace[2] / host_trace[5],
            host_trace[3] / host_trace[5], host_trace[4] / host_trace[5], host_waits);
  delete copy_pool;
  if (copy_stream) hipStreamDestroy(copy_stream);
  if (copy_stream2) hipStreamDestroy(copy_stream2);
  if (copy_join) hipEventDestroy(copy_join);
}

// ring of staging slots, (re)sized to the camera
static int host_ring_prepare(tf_volume* v) {
  HostFrames& hf = v->hf;
  const size_t npix = (size_t)v->cam.W * v->cam.H;
  if (hf.hslot_pixels == npix && hf.copy_stream) return TF_OK;
  hf.hslot_pixels = 0;  // not ready until every slot below fits
  TF_HIP(hipStreamSynchronize(v->stream));
  if (!hf.copy_stream) TF_HIP(hipStreamCreateWithFlags(&hf.copy_stream, hipStreamNonBlocking));
  TF_HIP(hipStreamSynchronize(hf.copy_stream));
  int rc;
  for (HostFrames::HostSlot& s : hf.hslot) {
    if ((rc = fit(s.h, npix * 8, v->stream)) || (rc = fit(s.d, npix * 12, v->stream))) return rc;
    if (!s.copied) TF_HIP(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    s.free_when = 0;  // (both streams were drained above)
  }
  if (!v->h_progress) {
    if ((rc = v->h_progress.alloc(64))) return rc;
    *v->h_progress.as<uint32_t>() = v->progress_seq;
  }
  hf.hslot_pixels = npix;
  hf.hslot_next = 0;
  return TF_OK;
}

void host_slot_release(tf_volume* v, int slot) {
  v->hf.hslot[slot].free_when = v->progress_seq + 1u;  // through = a later frame launch has started
}
// a frame of the ring has been enqueued: its staging slot is free when the last launch that reads its device images is
// through -- the frame's own launch, or the one that carries its pending patch stage (patch_launched releases it then)
static int host_slot_done(tf_volume* v, int slot) {
  AtlasState::PendPatch& pp = v->atlas.pend_patch;
  if (pp.on && pp.host_slot < 0) pp.host_slot = slot;
  else host_slot_release(v, slot);
  return TF_OK;
}

// Blocks until the last launch that reads a staging slot's device images is through.  No stream event: the frame
// launches stamp tf_volume::h_progress when they start.  The launch that follows the slot's last reader is normally on
// the stream already (the entry point runs kHostDefer frames behind); if none comes (the caller changed entry points),
// the stream is drained instead.
static int host_slot_wait(tf_volume* v, HostFrames::HostSlot& s) {
  if (!s.free_when) return TF_OK;
  volatile uint32_t* p = v->h_progress.as<uint32_t>();
  if ((int32_t)(v->progress_seq - s.free_when) < 0) {  // no launch that would stamp it is on the stream
    TF_HIP(hipStreamSynchronize(v->stream));
    s.free_when = 0;
    return TF_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; ++spin) {
    if ((int32_t)(*p - s.free_when) >= 0) break;
    if (poll_sleep_us() > 0) { std::this_thread::sleep_for(std::chrono::microseconds(poll_sleep_us())); continue; }
    __builtin_ia32_pause();
    if ((spin & 1023u) == 1023u) {
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      if (us > 20000.0) { TF_HIP(hipStreamSynchronize(v->stream)); break; }  // (a stalled device: fail through the API)
      if (us > 200.0) sched_yield();
    }
  }
  s.free_when = 0;
  return TF_OK;
}

// the H2D copy of a staged host frame must be through before a launch reads its device images: nothing to do when the
// copy event is already complete (the usual case: the entry point runs behind), otherwise the stream waits for it
static int host_copy_ready(tf_volume* v, HostFrames::Pending* p) {
  if (p->copied) return TF_OK;
  hipEvent_t ev = v->hf.hslot[p->slot].copied;
  const hipError_t q = hipEventQuery(ev);
  if (q == hipErrorNotReady) {
    TF_HIP(hipStreamWaitEvent(v->stream, ev, 0));
    v->hf.host_waits += 1;
  } else if (q != hipSuccess) {
    TF_HIP(q);
  }
  p->copied = true;
  return TF_OK;
}

// Launches the oldest of the m = n_pend pending frames; the min(2, m - 1) frames behind it ride on the launch as
// selection-only roles (K-A(f) | K-C(f+1) | K-B(f+2), like the streaming entry points).  The caller has made their copies
// ready (host_copy_ready).  The queue is empty while enqueue_frames runs: helpers below it may pass through TF_DEV, and
// there must be nothing for them to flush while this launch is being put together.
static int launch_window(tf_volume* v) {
  HostFrames& hf = v->hf;
  const int m = hf.n_pend, ahead = m - 1 < 2 ? m - 1 : 2;
  const HostFrames::Pending* p = hf.pend;
  const float* dd[3];
  const uint8_t* dc[3];
  float poses[36];
  for (int j = 0; j <= ahead; ++j) { dd[j] = p[j].d; dc[j] = p[j].c; memcpy(poses + 12 * j, p[j].pose, 48); }
  const TexturedArgs tex{p[0].pinv, p[0].fid};
  const int slot = p[0].slot;
  hf.n_pend = 0;
  const int rc = enqueue_frames(v, 1, ahead, dd, dc, poses, p[0].tex ? &tex : nullptr);
  for (int k = 1; k < m; ++k) hf.pend[k - 1] = hf.pend[k];
  hf.n_pend = m - 1;
  return rc ? rc : host_slot_done(v, slot);
}

int flush_deferred(tf_volume* v) {
  HostFrames& hf = v->hf;
  const int n = hf.n_pend;
  if (!n) return TF_OK;
  const float* const last_d = hf.pend[n - 1].d;
  const uint8_t* const last_c = hf.pend[n - 1].c;
  int rc = TF_OK;
  for (int k = 0; k < n && !rc; ++k) rc = host_copy_ready(v, &hf.pend[k]);
  while (hf.n_pend && !rc) rc = launch_window(v);
  hf.n_pend = 0;  // (an error drops what was still pending)
  return rc ? rc : bind_frame(v, last_d, last_c);
}

// rgb != nullptr: the colour image comes as Frame::rgb (3 bytes per pixel) with Frame::colorValidFlag (or none: every pixel
// valid) -- the inputs of the caller's own RGBA staging loops (MobileFusion.cpp:144-163, :232-243), which then run on the
// device behind the upload, on the copy stream
static int integrate_frame_host_impl(tf_volume* v, const float* depth, const uint8_t* rgba, const uint8_t* rgb,
                                     const uint8_t* color_valid, const float pose[12], const float* pose_inv16, int32_t frame_id) {
  if (!v || !depth || !pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (pose_inv16 && !rgba && !rgb) { set_error("the textured unit needs a colour image"); return TF_ERR_INVALID; }
  TF_DEV_NOFLUSH(v);
  int rc = host_ring_prepare(v);
  if (rc) return rc;
  HostFrames& hf = v->hf;
  // per-phase host time (five clock reads per call): tf_host_frame_times; TF_HOST_TRACE=1 prints it at destroy
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto lap = [&](int k, std::chrono::steady_clock::time_point& t) {
    const auto t1 = now();
    hf.host_trace[k] += std::chrono::duration<double, std::micro>(t1 - t).count();
    t = t1;
  };
  auto t = now();
  // The launch pipeline of the streaming entry points, kept alive across per-frame calls: this call integrates the
  // frame that arrived kHostDefer = FOUR calls ago, and that launch carries the selection stages of the two frames behind
  // it (K-A(f-4) | K-C(f-3) | K-B(f-2)); frames f-1 and f are only staged and copied.  A copy therefore has a whole
  // call's time to finish before a launch needs it, so the host finds the copy event complete and no wait goes into
  // the stream (a cross-stream wait ahead of a launch costs ~7 us of idle device; with three frames of deferral the
  // newest image a launch reads was uploaded by the call before, and 6-20 % of the launches still waited).  The deferral cannot be
  // observed: every other entry point flushes first (TF_DEV).
  // The launches go out FIRST where that costs nothing -- they need nothing of the new frame -- so that an idle device is
  // at work while this call stages and uploads (it starts ~45 us earlier: 2 % of a 20-frame window).
  const bool defer = hf.host_defer;
  constexpr int ND = HostFrames::kHostDefer;
  const float* bound_d = nullptr;
  const uint8_t* bound_c = nullptr;
  auto launch_oldest = [&]() -> int {
    if (!(defer && hf.n_pend == ND)) return TF_OK;
    for (int k = 0; k < 3; ++k) { rc = host_copy_ready(v, &hf.pend[k]); if (rc) return rc; }  // the launch reads the oldest frame and the two behind it
    bound_d = hf.pend[0].d;
    bound_c = hf.pend[0].c;
    rc = launch_window(v);
    if (rc) return rc;
    lap(4, t);
    hf.host_trace[5] += 1.0;
    return TF_OK;
  };
  // ... but only when they would not wait: the launch also reads the images of the two frames behind the oldest one
  // (selection roles), and the newest of those was uploaded by the PREVIOUS call.  On an idle device (the start of a
  // stream, a caller that paces its frames) that copy is through and the launches go out at once; in a saturated stream
  // it is a few microseconds old -- launching now would put a wait for it into the stream (7 us of idle device per
  // frame, run 46), launching behind the staging copy finds it complete.
  bool early = false;
  if (defer && hf.n_pend == ND) {
    const HostFrames::Pending& newest = hf.pend[2];  // (the newest frame the launch reads)
    early = newest.copied || hipEventQuery(hf.hslot[newest.slot].copied) == hipSuccess;
  }
  if (early) { rc = launch_oldest(); if (rc) return rc; }
  const size_t npix = hf.hslot_pixels;
  const int slot_index = hf.hslot_next;
  HostFrames::HostSlot& s = hf.hslot[slot_index];
  hf.hslot_next = (hf.hslot_next + 1) % HostFrames::kHostRing;
  // the kernels that read this slot's device images and the upload out of its pinned buffer have finished
  rc = host_slot_wait(v, s);
  if (rc) return rc;
  lap(0, t);
  TF_HIP(hipEventSynchronize(s.copied));
  lap(1, t);
  uint8_t* const sd = s.d.as<uint8_t>();
  uint8_t* const sh = s.h.as<uint8_t>();
  // the frame's host parts and where they go, in the pinned slot and in the device slot alike
  struct Seg { const void* src; size_t bytes, at; };
  Seg seg[3] = {{depth, npix * 4, 0}};
  int ns = 1;
  if (rgba) seg[ns++] = {rgba, npix * 4, npix * 4};
  if (rgb) seg[ns++] = {rgb, npix * 3, npix * 4};
  if (rgb && color_valid) seg[ns++] = {color_valid, npix, npix * 7};
  // images inside registered caller buffers (tf_host_register) go up straight from there
  bool direct = !hf.host_ranges.empty();
  for (int k = 0; k < ns && direct; ++k) direct = hf.registered(seg[k].src, seg[k].bytes);
  if (!direct) {  // parts composed in tf_host_frame_buffers' slot are where they belong already: no copy
    void* dst[3];
    const void* src[3];
    size_t nb[3];
    int nr = 0;
    for (int k = 0; k < ns; ++k)
      if (seg[k].src != sh + seg[k].at) { dst[nr] = sh + seg[k].at; src[nr] = seg[k].src; nb[nr++] = seg[k].bytes; }
    if (nr) {
      if (!hf.copy_pool) {
        const char* e = getenv("TF_COPY_THREADS");
        int helpers = e ? atoi(e) : 7;
        if (helpers < 0) helpers = 0;
        if (helpers > 15) helpers = 15;
        // helpers run where the scheduler puts them (on a shared host pinned helpers gave 1 run in 3 a 10-ms stall --
        // 100.8 us per frame at best, 150+ at worst, against a steady 102.6 unpinned; profiles/r3, run 36)
        const int pin = 0;
        static const int spin_us = getenv("TF_COPY_SPIN_US") ? atoi(getenv("TF_COPY_SPIN_US")) : 200;
        hf.copy_pool = new CopyPool(helpers, pin, spin_us);
      }
      hf.copy_pool->copy(dst, src, nb, nr);
    }
  }
  lap(2, t);
  if (direct) {
    // (depth and colour are two caller arrays = two copies.  The link moves 2.46 MB as ONE copy in 53 us -- 46 GB/s,
    // allocated page-locked or page-locked in place alike, tools/h2d_probe.py --; as two copies of 1.2 MB it takes 60 us when
    // they travel side by side on two copy queues and 66 us one behind the other on one queue (profiles/r5/README.md).  A
    // kernel that fetches the images itself -- 16-byte loads out of the mapped pages -- was no faster than the DMA
    // transfers and slowed the step kernels it ran next to: 100 -> 125 us per frame, profiles/r4/README.md)
    if (rgba) {  // seg[1] goes first, on the second copy queue
      if (!hf.copy_stream2) {
        TF_HIP(hipStreamCreateWithFlags(&hf.copy_stream2, hipStreamNonBlocking));
        TF_HIP(hipEventCreateWithFlags(&hf.copy_join, hipEventDisableTiming));
      }
      TF_HIP(hipMemcpyAsync(sd + seg[1].at, seg[1].src, seg[1].bytes, hipMemcpyHostToDevice, hf.copy_stream2));
      TF_HIP(hipEventRecord(hf.copy_join, hf.copy_stream2));
    }
    for (int k = 0; k < ns; ++k)
      if (!(rgba && k == 1)) TF_HIP(hipMemcpyAsync(sd + seg[k].at, seg[k].src, seg[k].bytes, hipMemcpyHostToDevice, hf.copy_stream));
    if (rgba) TF_HIP(hipStreamWaitEvent(hf.copy_stream, hf.copy_join, 0));
  } else {
    // (the parts of a STAGED frame go up as one copy on one copy stream: two streams -- two SDMA queues -- helped a
    // TSDF-only stream in steady state on a quiet host, 62 -> 52-54 us per frame, and doubled the first window behind resident
    // frames on a shared one; profiles/r4/README.md, run s13)
    TF_HIP(hipMemcpyAsync(sd, sh, seg[ns - 1].at + seg[ns - 1].bytes, hipMemcpyHostToDevice, hf.copy_stream));
  }
  if (rgb) {  // rgba = valid ? (r, g, b, 1) : 0, behind the upload on the copy stream (null flags: every pixel valid)
    launch_pack_rgba(sd + npix * 4, color_valid ? sd + npix * 7 : nullptr, reinterpret_cast<uchar4*>(sd + npix * 8), (uint32_t)npix,
                     hf.copy_stream);
    TF_HIP(hipGetLastError());
  }
  TF_HIP(hipEventRecord(s.copied, hf.copy_stream));
  lap(3, t);
  hf.last_upload = s.copied;
  if (!early) { rc = launch_oldest(); if (rc) return rc; }
  HostFrames::Pending& cur = hf.pend[hf.n_pend++];
  cur.d = reinterpret_cast<const float*>(sd);
  cur.c = rgba ? sd + npix * 4 : (rgb ? sd + npix * 8 : nullptr);
  memcpy(cur.pose, pose, sizeof(cur.pose));
  cur.tex = pose_inv16 != nullptr;
  if (pose_inv16) memcpy(cur.pinv, pose_inv16, sizeof(cur.pinv));
  cur.fid = frame_id;
  cur.slot = slot_index;
  cur.copied = false;
  // the caller's buffers are its own again when the call returns: an upload straight out of them must be through -- unless
  // the caller took that on itself (tf_host_frame_set_async: it calls tf_host_frame_fence before it touches a buffer again)
  if (direct && !hf.host_async) {
    auto tw = now();
    for (uint32_t spin = 0; hipEventQuery(s.copied) == hipErrorNotReady; ++spin) {
      if (poll_sleep_us() > 0) std::this_thread::sleep_for(std::chrono::microseconds(poll_sleep_us()));
      else if ((spin & 63u) == 63u) __builtin_ia32_pause();
    }
    lap(1, tw);
    cur.copied = true;
  }
  if (defer) return bound_d ? bind_frame(v, bound_d, bound_c) : TF_OK;
  // no deferral: integrate at once -- two selection-only launches per frame, the stream waits for the copy
  const float* const d = cur.d;
  const uint8_t* const c = cur.c;
  rc = host_copy_ready(v, &cur);
  if (rc) hf.n_pend = 0;
  else rc = launch_window(v);
  return rc ? rc : bind_frame(v, d, c);
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_host_frame_set_deferral(tf_volume* v, int on) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV(v);  // (frames still in the pipeline go onto the stream under the old setting)
  v->hf.host_defer = on != 0;
  return TF_OK;
}

int tf_host_frame_set_async(tf_volume* v, int on) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  v->hf.host_async = on != 0;
  return TF_OK;
}
int tf_host_frame_fence(tf_volume* v) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV_NOFLUSH(v);
  if (v->hf.last_upload) TF_HIP(hipEventSynchronize(v->hf.last_upload));  // (uploads of one handle complete in order)
  return TF_OK;
}

int tf_host_frame_deferral(tf_volume* v, int32_t* frames_behind, int32_t* ring_slots) {
  // (a null handle answers for a handle as tf_volume_create makes it: TF_HOST_DEFER=0 in the environment turns the deferral
  // off for every new handle, tf_host_frame_set_deferral for one)
  const bool defer = v ? v->hf.host_defer : host_defer_default();
  if (frames_behind) *frames_behind = defer ? HostFrames::kHostDefer : 0;
  if (ring_slots) *ring_slots = HostFrames::kHostRing;
  return TF_OK;
}

int tf_host_register(tf_volume* v, const void* p, int64_t bytes) {
  if (!v || !p || bytes <= 0) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_NOFLUSH(v);
  const uint8_t* b = static_cast<const uint8_t*>(p);
  if (v->hf.registered(b, (size_t)bytes)) return TF_OK;  // already inside a range of this handle
  std::lock_guard<std::mutex> lk(g_locked_mu);
  const LockedRanges::Answer a = g_locked.acquire(b, (size_t)bytes);
  if (a.what == LockedRanges::kOverlap) {
    set_error("tf_host_register: the buffer overlaps a range that is page-locked already with a different extent "
              "(register the whole arena once, or ranges that do not overlap)");
    return TF_ERR_INVALID;
  }
  if (a.what == LockedRanges::kLockNew) {
    auto lock = [&]() -> int { TF_HIP(hipHostRegister(const_cast<uint8_t*>(b), (size_t)bytes, hipHostRegisterDefault)); return TF_OK; };
    if (lock()) { g_locked.release(b); return TF_ERR_HIP; }
  }
  v->hf.host_ranges.push_back({b, (size_t)bytes, a.base});
  return TF_OK;
}
int tf_host_unregister(tf_volume* v, const void* p) {
  if (!v || !p) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV(v);  // (frames still in the entry point's pipeline have been uploaded; their launches go out now)
  HostFrames& hf = v->hf;
  TF_HIP(hipStreamSynchronize(hf.copy_stream ? hf.copy_stream : v->stream));
  for (size_t i = 0; i < hf.host_ranges.size(); ++i)
    if (hf.host_ranges[i].p == static_cast<const uint8_t*>(p)) {
      const uint8_t* locked = hf.host_ranges[i].locked;
      hf.host_ranges.erase(hf.host_ranges.begin() + (long)i);
      return host_range_release(locked);
    }
  set_error("not a registered buffer");
  return TF_ERR_INVALID;
}

int tf_host_frame_times(tf_volume* v, double out[7], int reset) {
  if (!v || !out) { set_error("null argument"); return TF_ERR_INVALID; }
  HostFrames& hf = v->hf;
  out[0] = hf.host_trace[5];  // calls that put their oldest pending frame's launches on the stream (flushes do not count)
  for (int k = 0; k < 5; ++k) out[1 + k] = hf.host_trace[k];  // us: waiting for the device to free a slot | waiting for the slot's last upload | staging copy | upload enqueue | launches
  out[6] = (double)hf.host_waits;  // launches that had to wait in the stream for an upload
  if (reset) { for (int k = 0; k < 6; ++k) hf.host_trace[k] = 0.0; hf.host_waits = 0; }
  return TF_OK;
}

int tf_host_frame_buffers(tf_volume* v, float** depth, uint8_t** rgba) {
  if (!v || !depth || !rgba) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_NOFLUSH(v);
  int rc = host_ring_prepare(v);
  if (rc) return rc;
  HostFrames::HostSlot& s = v->hf.hslot[v->hf.hslot_next];
  TF_HIP(hipEventSynchronize(s.copied));  // the previous upload out of this slot has left the host buffer
  *depth = s.h.as<float>();
  *rgba = s.h.as<uint8_t>(v->hf.hslot_pixels * 4);
  return TF_OK;
}

int tf_integrate_frame_host(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                            const float* pose_inv16, int32_t frame_id) {
  return integrate_frame_host_impl(v, depth, rgba, nullptr, nullptr, pose, pose_inv16, frame_id);
}
int tf_integrate_frame_host_rgb(tf_volume* v, const float* depth, const uint8_t* rgb, const uint8_t* color_valid,
                                const float pose[12], const float* pose_inv16, int32_t frame_id) {
  if (!rgb) { set_error("null colour image (tf_integrate_frame_host takes depth-only frames)"); return TF_ERR_INVALID; }
  return integrate_frame_host_impl(v, depth, nullptr, rgb, color_valid, pose, pose_inv16, frame_id);
}

}  // extern "C"
