// tf_volume.h -- host-side state behind the opaque tf_volume handle.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tf_fusion.h"
#include "tf_device.h"
#include "tf_host_frames.h"
#include "tf_mem.h"

namespace tf {

void set_error(const std::string& msg);

#define TF_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      ::tf::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
      return TF_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)

// Every C-ABI entry point binds the calling thread to the handle's device first: scratch allocations,
// launches and copies must land on the GPU the volume lives on, whatever device the caller's thread
// had current (two volumes on different GPUs in one process, framework worker threads).
#define TF_DEV_NOFLUSH(v)                                                                   \
  do {                                                                                      \
    ++(v)->call_seq;                                                                        \
    ++(v)->model_gen;                                                                       \
    hipError_t _e = hipSetDevice((v)->device);                                              \
    if (_e != hipSuccess) {                                                                 \
      ::tf::set_error(std::string("hipSetDevice: ") + hipGetErrorString(_e));               \
      return TF_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)
// Every entry point but tf_integrate_frame_host first brings the frames that entry point has deferred (it runs
// HostFrames::kHostDefer frames behind its caller, see tf_host_frames.cpp) onto the stream, so that nothing can observe the deferral.
#define TF_DEV_STREAM(v)                                                                    \
  do {                                                                                      \
    TF_DEV_NOFLUSH(v);                                                                      \
    if ((v)->hf.n_pend) {                                                                   \
      int _rc = ::tf::flush_deferred(v);                                                    \
      if (_rc) return _rc;                                                                  \
    }                                                                                       \
  } while (0)
// ... and, except for the streaming entry points (whose next launch carries it), the patch stage of the last
// textured frame (AtlasState::pend_patch).
#define TF_DEV(v)                                                                           \
  do {                                                                                      \
    TF_DEV_STREAM(v);                                                                       \
    if ((v)->atlas.pend_patch.on) {                                                         \
      int _rc = ::tf::patch_flush(v);                                                       \
      if (_rc) return _rc;                                                                  \
    }                                                                                       \
  } while (0)

// The model generation (tf_volume::model_gen) decides whether the resident model stream (ModelState) is current.  It is
// advanced by EVERY entry point -- TF_DEV_NOFLUSH above -- except the few that enter through TF_DEV_READER: calls that
// provably change no mesh, no patch and no pool slot (tf_model_stream_*, tf_render_*, tf_raycast*, tf_query_points*,
// tf_align_*, tf_sync).  A reader that is not on that list costs one repack; a writer cannot be forgotten.  A reader that has to bring
// deferred frames or a pending patch stage onto the stream first is a writer for that call.
#define TF_DEV_READER(v)                                                                    \
  do {                                                                                      \
    const uint64_t _gen = (v)->model_gen;                                                   \
    const bool _writes = (v)->hf.n_pend || (v)->atlas.pend_patch.on;                        \
    TF_DEV(v);                                                                              \
    if (!_writes) (v)->model_gen = _gen;                                                    \
  } while (0)

// Scratch pool: a device half and a pinned host half, two fitted buffers (tf_mem.h) that reserve() grows on demand to a
// power of two, draining the handle's stream first.  The halves grow independently: growing the host half never frees the
// device half (which may hold the dirty list tf_compress_meshes takes over, tf_volume::dirty_list_seq).  `s = Scratch{}`
// gives both back.
struct Scratch {
  DevMem d;
  PinMem h;
};
int reserve(tf_volume* v, Scratch& s, size_t dev_bytes, size_t host_bytes);

// Byte layout of a staging area: each block at a 16-byte aligned offset; size = the total.
struct Layout {
  size_t size = 0;
  size_t take(size_t bytes) {
    const size_t at = size;
    size = (size + bytes + 15) & ~(size_t)15;
    return at;
  }
};

// Typed arrays carved out of a block in Layout's steps (base == null: only the size is wanted, every pointer is null).
struct Carver {
  uint8_t* base;
  Layout L;
  explicit Carver(void* b) : base(static_cast<uint8_t*>(b)) {}
  template <typename T> void take(T*& p, size_t count) {
    const size_t at = L.take(count * sizeof(T));
    p = base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

// Host and device base of a staging area in a pool.
struct Stage {
  uint8_t* h = nullptr;
  uint8_t* d = nullptr;
  template <typename T> T* hp(size_t at) const { return reinterpret_cast<T*>(h + at); }
  template <typename T> T* dp(size_t at) const { return reinterpret_cast<T*>(d + at); }
};
// Reserves the pool, then synchronises the stream once: an earlier call may still read or write the pool.
int stage_begin(tf_volume* v, Scratch& s, size_t dev_bytes, size_t host_bytes, Stage* st);
// Host bytes in at offset `at` of the staging area, and their upload to the same offset of the device half (enqueued).
int stage_in(tf_volume* v, const Stage& st, size_t at, const void* src, size_t bytes);
// `bytes` at offset `at` of the device half back into the host half, one wait, and from there to out (null: left there).
int stage_out(tf_volume* v, const Stage& st, size_t at, size_t bytes, void* out);
// stage_begin for `bytes` on both halves, then ids (host, int32[3n]) as an int4 list at offset 0, its upload enqueued.
int stage_ids(tf_volume* v, Scratch& s, size_t bytes, const int32_t* ids, int64_t n, Stage* st);
// The first m entries of the int4 list at the start of the pool's device half -> out (int32[3m]); returns after the copy.
int download_ids(tf_volume* v, const Scratch& s, int64_t m, int32_t* out);
// int32[3n] -> int4[n] (w: the fourth word per id, or 0), and back.
void pack_ids(const int32_t* ids, int64_t n, int32_t* out4, const int* w = nullptr);
void unpack_ids(const int32_t* in4, int64_t n, int32_t* ids);
// set_error("chunk (x,y,z) <what>") for entry i of ids; returns TF_ERR_MISSING_CHUNK
int missing_chunk_error(const int32_t* ids, int64_t i, const char* what);

struct ProfEvent {
  hipEvent_t a, b;
  int kind;
};

struct KeyframeSlot {
  DevMem rgb, depth;  // tf_keyframe_cache's copies, u8[H][W][3] and f32[H][W], fitted to the camera; empty: the caller's images
  int slot = -1;      // entry of the device keyframe table
  bool has_pose = false;  // tf_keyframe_set_pose has been called (the table's pose is the identity until then)
};

struct AtlasState {
  int32_t aw = 13824, ah = 13824;
  uint64_t pw = 0, ph = 0;
  DevMem buf;    // VolumeDev::atlas, u8[ah][aw][3]
  DevMem block;  // everything else of VolumeDev's atlas part, carved (atlas_init)
  // keyframe table (device copy + host mirror)
  std::unordered_map<int32_t, KeyframeSlot> keyframes;
  std::vector<KfDev> h_kf;
  std::vector<uint8_t> kf_used;
  int kf_cap = 0;
  PinMem h_dirty_len;  // one u32, device-visible: the mesher's filter leaves the length of a frame's dirty list here
  int fused_par = 0;   // counter set of the next fused frame
  // fused flow: the patch stage of textured frame f (slot hand-out, CompressMeshes' exchange, CalculateTexCoords,
  // UpdateBuffer) is not launched behind the frame's mesher but rides on the NEXT frame's launch, next to its voxel
  // update (k_frame, tf_kernels.hip) -- it reads meshes, the frame's own images and the atlas, nothing K-A touches.
  // Anything that could observe the deferral flushes it first (TF_DEV -> patch_flush: the stage as a launch of its own).
  struct PendPatch {
    bool on = false;
    PatchStage st;
    int host_slot = -1;  // tf_integrate_frame_host: the staging slot whose device images the stage still reads
  } pend_patch;
  bool fused_armed = false;  // the counter sets are in the state the fused flow expects
  // tf_texture_frame_device_phase: phase 1 (dirty set + interior meshes) of the stage of frame `phase1_epoch` has run,
  // phase 2 (boundary meshes behind the caller's unpack, pending patch stage) has not
  bool phase1_on = false;
  uint32_t phase1_epoch = 0;
  Scratch stage;  // the atlas entry points' own pool (they leave tf_volume::scratch alone)
};

// Host side of the resident TexMap (tf_volume::tm, tf_texmap.hip): what the host has to know without asking the device.
struct TexMapState {
  std::vector<int32_t> kf_row;       // kflist[r].keyFrameIndex of the last tf_texmap_set_keyframes
  std::vector<int32_t> kf_inv;       // frame index -> row, -1 = none (frameIndexToKeyframeDB, MobileFusion.cpp:293-296)
  // device copy of kf_row + 64 spare words (the tail's keyframes to update), pinned staging of the uploads and their event
  Scratch kf;
  hipEvent_t kf_ev = nullptr;
  int64_t nodes_bound = 0;           // chunks ever handed to tf_texmap_update: an upper bound of the node count
  DevMem block;                      // the map's device block (tm_arrays): what tf_volume::tm's pointers point into
  PinMem h_ctl;                      // a TexMapCtl: the control block as read back; there whenever the map's device block is
  // the problem assembled last: per-node arrays (pn, room for pn_cap nodes), per-label arrays (pz, pz_cap labels); device halves
  Scratch pn, pz;
  size_t pn_cap = 0, pz_cap = 0;
  int64_t n = 0, nnz = 0;            // its size
  // tf_texture_tail_device: chunksToUpdate as a device list (raw = as the dirty set gave it, ctu = ascending chunk id);
  // one allocation, d_ctu behind d_ctu_raw
  DevMem ctu;
  int4* d_ctu = nullptr;
  int64_t ctu_n = 0;                 // its length, known since the tail's one wait
};

// Device-resident CompensateColor (tf_cc.hip): its list, cluster table and partial sums in one block, null until first use
struct CcState {
  DevMem block;
};

// The state block of an aligner (tf_align.hip, tf_align_color.hip, tf_align_group.hip, tf_align_icp.hip): partial sums, the
// f64 poses, control words, the log -- sized for the camera at stride 1, null until first use.  Each aligner has its own,
// so that its log outlives the others' calls.
struct AlignBlock {
  DevMem block;
  size_t cap_tiles = 0;  // 8 x 8 pixel tiles the block has room for
};
// The projective ICP's block, and the six planes of the model's vertex and normal maps of the forms that raycast
// themselves (null until one of those is used); the normal-compatibility gate of tf_align_icp_set_gate (off in a new state,
// so off again after tf_volume_reset); the depth pyramid of tf_align_icp_set_pyramid (off in a new state too) with what a
// call with it on needs beside `maps`: the images of levels 1 to 3, their model maps, and the level-sized maps
// tf_align_icp_residuals spreads over the full image -- each grown on demand (tf_align_icp_pyramid.hip)
struct AlignIcpState {
  AlignBlock st;
  DevMem maps;
  size_t map_pixels = 0;  // pixels each plane of `maps` has room for
  bool gate_on = false;
  tf_align_icp_gate gate{};
  bool pyr_on = false;
  tf_align_icp_pyramid pyr{};
  DevMem pyr_img, pyr_maps, pyr_res;  // fitted buffers (tf_mem.h)
};

// The colour ICP's block (tf_align_icp_color.hip), and ten planes of f32 beside it: the model's vertex and normal maps of
// the form that raycasts itself (six), then the model maps L, Gu, Gv and Z of a call (four) -- null until first use
struct AlignIcpColorState {
  AlignBlock st;
  DevMem maps;
  size_t map_pixels = 0;  // pixels each plane of `maps` has room for
};

// Exposure compensation of the photometric aligners (tf_align_exposure.hip): the setting of tf_align_set_exposure (off in a
// new state, so off again after tf_volume_reset), the cell that holds the start pair (two f64: gain, offset), and one state
// block per aligner (0: tf_align_color.hip's calls, 1: tf_align_icp_color.hip's) with the pair between iterations, the log
// and three rows of partial sums per workgroup.  ran[w]: the aligner's last call ran with the setting on.
struct AlignExposureState {
  bool on = false;
  tf_align_exposure e{};
  DevMem cell;
  AlignBlock st[2];
  bool ran[2] = {false, false};
  bool hold_carry = false;  // tf_track_frame_color's first stage: the estimate goes to the cell whatever carry says
};

// Relocalisation against the cached keyframes (tf_reloc.hip): the configuration, and the index -- one block holding every
// row's descriptor, the query's and the scores; the host keeps which keyframe a row belongs to.  Empty until configured.
struct RelocState {
  bool on = false;
  tf_reloc_params p{};
  int W = 0, H = 0;      // the camera the configuration was made for
  DevMem block;
  size_t cap_rows = 0;   // rows the block has room for
  std::vector<int32_t> kf_ids;                   // row -> keyframe id
  std::unordered_map<int32_t, int32_t> row_of;   // keyframe id -> row
};

// The model's DrawMeshes stream, resident in the handle (tf_model.hip): packed on the device, counts in device words,
// kept until the model changes.  Everything is empty until first use; `ModelState{}` gives it all back.
struct ModelState {
  DevMem vtx;    // f32[cap_v][12]
  DevMem idx;    // u32[cap_i]
  DevMem list;   // the complete() patches as listed | the same in ascending chunk key, [max_chunks] each
  DevMem rank;   // u32[max_chunks] rank of every listed patch
  DevMem rec;    // DrawPatch[max_chunks] in rank order
  DevMem ctl;    // u32[8] the control block tf_model_stream_get hands out, u32[8] the pack's own words behind it
  PinMem h_ctl;  // the control block as the synchronous update reads it back
  int64_t cap_v = 0, cap_i = 0;  // capacity in vertices / indices (0: none yet)
  bool packed = false;           // a pack is on the stream (or through) ...
  uint64_t gen = 0;              // ... and this was tf_volume::model_gen when it was enqueued
  bool counted = false;          // the host has read that pack's counts: nv / ni
  int64_t nv = 0, ni = 0;
  uint64_t packs = 0, hits = 0;  // tf_model_stream_stats
};

// RCCL communicator of the handle (tf_comm_init) and the exchange buffers
struct CommState {
  void* comm = nullptr;  // ncclComm_t
  int rank = 0, nranks = 0;
  DevMem send, recv;
  int64_t cap_records = 0;
  int mode = TF_XCHG_NEIGHBOURS;
  uint64_t exchanges = 0, bytes_received = 0, bytes_sent = 0;  // tf_comm_stats / tf_comm_stats_ex
  uint64_t bound_records = 0;  // sum of the record capacities the sized exchanges were given (sent sides)
  bool neighbours_ok = false;  // tf_comm_check_partition found every slab wide enough and rank-ordered
  bool checked = false;
};
// the sized exchange's record capacity for a band with c selected chunks: multiples of 8 records, at least 8 (room
// for what an earlier, overflowing exchange left flagged), never more than the caller's cap
inline uint32_t xchg_bucket(uint32_t c, int64_t cap) {
  uint64_t b = ((uint64_t)c + 7u) & ~7ull;
  if (b < 8) b = 8;
  if (cap > 0 && b > (uint64_t)cap) b = (uint64_t)cap;
  return (uint32_t)b;
}

}  // namespace tf

struct tf_volume {
  static constexpr int kSelSets = 4;  // ring of selection sets: K-B / K-C run 2 / 1 frames ahead of K-A
  tf_config cfg;
  int device = 0;
  float res = 0.005f;
  int use_color = 1;
  // camera as given (floats) and as consumed (int-truncated)
  float fx = 525.f, fy = 525.f, cx = 319.5f, cy = 239.5f;
  tf::Cam cam;
  // tf_raycast_camera: intrinsics (int-truncated) and image size of the raycaster; ray_w = 0 = the camera above
  float ray_fx = 0.f, ray_fy = 0.f, ray_cx = 0.f, ray_cy = 0.f;
  int ray_w = 0, ray_h = 0;
  tf::Integ ig;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  tf::VolumeDev dev;
  tf::SelBuf selbuf[kSelSets];  // ring of selection scratch sets (dev.sel = the active set)
  int cur_sel = 0;
  // frames whose selection stages already ran at the end of the previous streaming call (n_ahead)
  struct Primed { const float* depth; float pose[12]; };
  Primed primed[2];
  int n_primed = 0;
  std::vector<tf::DevMem> allocs;  // the fixed allocations of tf_volume_create
  // frame images: the staging targets of tf_frame_upload, one fitted buffer carved as depth | rgba | quality
  tf::DevMem images;
  // the per-frame host path (tf_integrate_frame_host, tf_host_*): staging ring, registered caller buffers, deferred frames
  tf::HostFrames hf;
  // Launch progress without stream events: every frame launch writes its sequence number into this pinned word when it
  // STARTS (= every launch ahead of it on the stream is through).  An event record between two launches of a frame cost
  // the host-frames path 6.8 us per frame of idle device time (profiles/r3, run 29).
  // Both stay here, not in HostFrames: launch_frame stamps them for every stream, host frames or not.
  tf::PinMem h_progress;  // one u32, null until the host ring is first prepared
  uint32_t progress_seq = 0;   // stamp of the last frame launch put on the stream
  tf::FrameImages frame{nullptr, nullptr, nullptr};
  bool frame_bound = false;
  // host shadow of the device-resident visible list (int32[3*n]); -1 = device list unknown
  std::vector<int32_t> host_list;
  int64_t host_list_n = -1;
  // what the device list's needsUpdate / isNew flags hold, as far as the call-by-call entry points know (valid while
  // host_flags_n == host_list_n): a caller that hands back the flags it was given -- the reference's loop over one
  // keyframe's frames does -- costs no upload
  std::vector<uint8_t> host_needs, host_new;
  int64_t host_flags_n = -2;
  // entry points counted (TF_DEV*): tf_compress_meshes reuses the dirty list tf_update_meshes left in scratch.d when that was
  // the call right before it (MobileFusion.cpp:327-345 calls them back to back; nothing in between can have marked a chunk)
  uint64_t call_seq = 0, dirty_list_seq = ~0ull;
  uint32_t dirty_list_n = 0;
  tf::PinMem h_ctl;  // pinned: FrameCtl head + VolCtl as fetch_ctl reads them
  uint32_t epoch = 0;        // finalize counter (mark / erase stamps are epoch + 1)
  uint32_t clear_floor = 0;  // stamps <= this were cleared (Chisel::CompressMeshes' chunksToUpdate.clear())
  uint32_t mesh_epoch = 0;   // meshing passes so far (MeshRec::epoch)
  int mesh_par = 0;          // parity of the next mesher launch (VolumeDev::mesh_cnt)
  tf::DevMem group;  // staging of tf_integrate_depth_group_host: six depth images
  tf::Scratch scratch;  // on-demand staging of the entry points (uploads / downloads, device scratch)
  // profiling
  bool prof_open = false;
  uint32_t prof_mask = 0;  // bit k = time kernels of kind TF_PROF_k
  std::vector<tf::ProfEvent> prof_events;
  std::vector<hipEvent_t> prof_pool;
  tf_profile prof_acc{};
  tf::AtlasState atlas;
  tf::CommState comm;
  tf::TexMapDev tm{};   // TexMap resident on the device: null pointers until the first tf_texmap_* call
  tf::TexMapState tmx;
  tf::CcState cc;
  tf::AlignBlock align, align_color, align_group;
  tf::AlignIcpState align_icp;
  tf::AlignIcpColorState align_icp_color;
  tf::AlignExposureState align_exposure;
  tf::RelocState reloc;
  tf::DevMem devpose;  // one PoseConsts (tf_devpose.h): what k_pose_consts derives from a pose cell; null until first use
  tf::DevMem devpose_inv;  // one PoseInverse: the cell's rigid inverse for the patch stage, written by the same launch
  tf::ModelState model;
  uint64_t model_gen = 0;  // advanced by every entry point that is not a whitelisted reader (TF_DEV_READER)
  int64_t comm_cap = 0;  // > 0: the fused textured flow exchanges the ghost band after every voxel update
  // band counts of a frame's selection as the host sees them: pinned words [0] tag (frame epoch + 1), [1..4] FrameCtl::band_cnt
  tf::PinMem h_xchg;  // u32[16], null until first use (xchg_words)
  uint32_t xchg_pub_enq = 0;  // frame tag of the publish that is already on the stream (0: none)
  uint32_t xchg_pub_seq = 0;  // ... the sequence number that publish writes into h_xchg[0] (what the host waits for)
  // the per-frame exchange overlapped with the interior meshes (texture_stage): second stream, fork / join events
  hipStream_t xstream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // tf_atlas_snapshot_rows: a second thread (the reference's GUI thread reads Atlas::texture_buffer while the map thread
  // writes it, GCFusion/MobileFusion.h:404-421) copies atlas rows out consistently.  atlas_mu orders that thread's
  // in-stream snapshot against the map thread's atlas-writing launches; atlas_seq counts those launches, atlas_frame is
  // the label of the newest one; snap_mu serialises readers (one snapshot buffer, one read stream).
  std::mutex atlas_mu, snap_mu;
  std::atomic<uint64_t> atlas_seq{0};
  std::atomic<int32_t> atlas_frame{-1};
  hipStream_t read_stream = nullptr;
  hipEvent_t read_ev = nullptr;
  tf::DevMem snap;
  bool xchg_overlap = true;        // tf_comm_exchange_overlap
  uint64_t xchg_overlapped = 0;    // exchanges that ran next to an interior mesh pass (tf_comm_stats_ex)
  uint32_t xchg_seq = 0;      // publish sequence numbers handed out (monotonic over the handle's life: a stale word never matches)
};

namespace tf {
// Around the enqueue of a launch that writes atlas texels: nothing of tf_atlas_snapshot_rows can land between the launch
// and the bump of the write sequence (label: Patch::frameid of what it writes, INT32_MIN = keep the last one).
struct AtlasWriteScope {
  tf_volume* v;
  int32_t label;
  AtlasWriteScope(tf_volume* vv, int32_t l) : v(vv), label(l) { v->atlas_mu.lock(); }
  ~AtlasWriteScope() {
    if (label != INT32_MIN) v->atlas_frame.store(label, std::memory_order_relaxed);
    v->atlas_seq.fetch_add(1, std::memory_order_release);
    v->atlas_mu.unlock();
  }
  AtlasWriteScope(const AtlasWriteScope&) = delete;
  AtlasWriteScope& operator=(const AtlasWriteScope&) = delete;
};
// stream synchronisation + control blocks; VolCtl::n_tmp as read (may be NULL); sticky status -> error code
int sync_status(tf_volume* v, uint32_t* n_tmp);
int launch_prepare(tf_volume* v, const Pose& pose, bool with_acquire, hipStream_t s = nullptr);  // tf_capi.cpp
struct KfStoreArgs;  // tf_kf_store.h
// ride_filter: a patch stage still pending when the stage starts rides on its filter launch (the keyframe unit: there is
// no k_frame launch for it to ride on) instead of going out as a launch of its own
int texture_stage(tf_volume* v, const SelBuf& sel, const FrameImages& img, uint32_t frame_epoch, const float* pose_inv16,
                  int32_t frame_id, bool claimed = false, const FrameCtl* next_ctl = nullptr, bool ride_filter = false,
                  bool sized_xchg = false, int phase = 0,   // sized_xchg: sel.ctl holds the frame's band counts (fused stream only)
                  const KfStoreArgs* store = nullptr);      // the keyframe unit: the list's validChunks store rides on the filter launch
int texture_stage_finish(tf_volume* v, const FrameImages& img, uint32_t frame_epoch, const float* pose_inv16, int32_t frame_id, int par);
// the four band counts of the frame whose selection wrote `ctl` (tag = its epoch + 1): waits for the device to publish them
int xchg_band_counts(tf_volume* v, const FrameCtl* ctl, uint32_t tag, uint32_t cnt[4], hipStream_t s = nullptr);
int xchg_words(tf_volume* v);  // tf_volume::h_xchg is there (allocated and zeroed on first use)
uint32_t nbr_next_seq(tf_volume* v);  // neighbour table: the seq of the filter launch about to go out (tf_capi.cpp)
// the dirty set (Chisel::meshesToUpdate) as a device list in scratch.d: [0,16) count word, ids from byte 16 (tf_mesh.hip)
int dirty_list_enqueue(tf_volume* v);
void launch_dirty_frame_store(const VolumeDev& v, int par, uint32_t stamp, const KfStoreArgs& a, hipStream_t s);  // tf_mesh.hip
struct PoseInverse;  // tf_devpose.h
// the pending patch stage as a launch of its own; d_inv: the frame's matrix is the one in that device block, where its gate
// is set (k_patch_posed), not the one the stage was armed with
int patch_flush(tf_volume* v, const PoseInverse* d_inv = nullptr);
// the pending patch stage has been put on the stream (as a role of a frame / filter launch or on its own)
int patch_launched(tf_volume* v);
// Software-pipelined enqueue of n frames (+ n_ahead selection-only ones) on the handle's stream, and the textured flow's
// per-frame arguments (tf_capi.cpp); bind_frame: tf_frame_bind_device without the entry checks
struct TexturedArgs {
  const float* pose_inv16;  // per frame: f32(SE3d.inverse().matrix()) of the frame's pose
  int32_t first_frame_id;
  // one frame whose pose is in device memory (tf_devpose.hip): pose_inv16 is not read, the frame's patch stage goes out
  // behind its mesher as a launch of its own that takes the matrix from this block, and nothing stays pending
  const PoseInverse* d_inv = nullptr;
};
int enqueue_frames(tf_volume* v, int64_t n, int64_t n_ahead, const float* const* d_depth, const uint8_t* const* d_rgba,
                   const float* poses12, const TexturedArgs* tex);
int bind_frame(tf_volume* v, const float* d_depth, const uint8_t* d_rgba);
int fused_arm(tf_volume* v);  // the fused flow's counter sets in their start state (no-op once armed)
void prof_begin(tf_volume* v, int kind, hipStream_t s = nullptr);
void prof_end(tf_volume* v, hipStream_t s = nullptr);
int atlas_init(tf_volume* v);
int atlas_reset(tf_volume* v);
int comm_exchange(tf_volume* v, int64_t cap_records, int dirty_par, uint32_t stamp, const FrameCtl* ctl = nullptr,
                  uint32_t tag = 0, const FrameCtl* next_ctl = nullptr, hipStream_t xs = nullptr);  // xs: the stream it runs on (null: the handle's)
// the pack launches of tf_boundary_pack_block / tf_boundary_pack_bands2 on a given stream (no deferred-frame flush: the caller did it)
int boundary_pack_block_on(tf_volume* v, void* d_block, int64_t cap_records, hipStream_t s);
int boundary_pack_bands2_on(tf_volume* v, void* d_block_down, int64_t cap_down, void* d_block_up, int64_t cap_up, hipStream_t s);
void comm_destroy(tf_volume* v);
int kf_push(tf_volume* v, int slot);
// the volume and the map as the map's kernels take them
inline TmDev tm_dev(const tf_volume* v) {
  TmDev d;
  static_cast<VolumeDev&>(d) = v->dev;
  d.tm = v->tm;
  return d;
}
void texmap_release(tf_volume* v);  // frees the resident TexMap (tf_texmap.hip); the handle is back at its footprint without one
// work entries [first offending entry, n) of the patch work list out of the stage: an entry with a mesh whose chunk is no node of
// the resident graph or whose label names no cached keyframe (tf_generate_patches_selected); w of the others = keyframe-table entry
void launch_tm_work_labels(tf_volume* v, uint32_t n, uint32_t* d_first_fail);
// tf_texture_tail_device's pieces outside tf_texmap.hip.  compress_device_list (tf_mesh.hip): CompressMeshes over the dirty set,
// the dirty keys that own a mesh appended to d_out (order free), their count copied to *d_count, the dirty set cleared;
// *bound = what the host knows about the count.  patch_stage_device (tf_atlas.hip): GeneratePatches with the resident labels
// and UpdateAtlas over a device list of n entries, nothing read back.
int compress_device_list(tf_volume* v, int4* d_out, uint32_t cap_out, uint32_t* d_count, uint32_t* bound);
int patch_stage_device(tf_volume* v, const int4* d_list, uint32_t n, uint32_t* d_first_fail);
// Chisel::CompensateColor enqueued on the handle's stream, nothing read back (tf_cc.hip); cc_release frees its buffers
int cc_enqueue(tf_volume* v, uint32_t* d_n_clusters);
void cc_release(tf_volume* v);
// The aligners' host side (tf_align.hip; the device side is tf_align_rows.h).  align_cam: the camera of the depth image,
// the one tf_raycast_camera set (any size), else the handle's.  align_check: what every aligner refuses a call for
// (with_iters: iters are read too).  track_check (tf_align_icp.hip): what tf_track_frame refuses a call for, for
// tf_relocalise to refuse it ahead of its first launch.
struct AlignCam { float fx, fy, cx, cy; int W, H; };
AlignCam align_cam(const tf_volume* v);
bool finite_all(const float* p, int n);
int align_check(tf_volume* v, const float* depth, const float* pose, const tf_align_params* p, bool with_iters);
int track_check(tf_volume* v, const float* depth, const float* pose, const tf_align_icp_params* icp_params,
                const tf_align_params* sdf_params);
size_t align_pixels(const tf_volume* v);  // of the camera
size_t align_tiles(const tf_volume* v);   // 8 x 8 tiles of the camera at stride 1
// First use, or a larger camera since: b.block (re)allocated to bytes_of(align_tiles(v)) after a wait for the stream, its
// first clear_bytes (the control words) zeroed.
int align_ensure(tf_volume* v, AlignBlock& b, size_t (*bytes_of)(size_t tiles), size_t clear_bytes);
// A level's geometry and parameters as the kernels read them (level == n_levels: the closing evaluation, at the last
// level's stride); sc->n_rows is the rows launch's grid.
struct AlignRowsCommon;
struct AlignSolveCommon;
void align_level(const tf_volume* v, const tf_align_params& p, int level, AlignRowsCommon* rc, AlignSolveCommon* sc);
// Its twin for a level that is an image of its own (the projective ICP's depth pyramid): cam is that image's camera, every
// pixel of it is a row (the rows' stride is 1, the grid is the image's), and the solve's block keeps the level's stride,
// so that a log record's stride still names the level's block.
void align_level_image(const AlignCam& cam, const tf_align_params& p, int level, AlignRowsCommon* rc, AlignSolveCommon* sc);
// The schedule of a call: evaluate(rc, sc) for iters[l] evaluations of every level l, then once to close.  level_cams !=
// null: a level of stride 2^k is the image of camera level_cams[k] (align_level_image).
void align_walk(const tf_volume* v, const tf_align_params& p,
                const std::function<void(const AlignRowsCommon&, const AlignSolveCommon&)>& evaluate,
                const AlignCam* level_cams = nullptr);
// tf_*_log: waits for the stream, reads the control words at d_ctl (null: no call yet, no records) and copies
// min(n_eval, cap) records of rec_bytes from d_log; *n = the records there are.
int align_log(tf_volume* v, const void* d_ctl, const void* d_log, size_t rec_bytes, void* out, int64_t cap, int64_t* n);
void align_release(tf_volume* v);        // these free the state block of tf_align.hip,
void align_color_release(tf_volume* v);  // of tf_align_color.hip,
void align_group_release(tf_volume* v);  // of tf_align_group.hip,
void align_icp_release(tf_volume* v);    // of tf_align_icp.hip with its maps,
void align_icp_color_release(tf_volume* v);  // of tf_align_icp_color.hip with its maps,
void align_exposure_release(tf_volume* v);   // and of tf_align_exposure.hip with its cell: the setting is off again
// what tf_align_frame_icp refuses a call for, but null map and result pointers (tf_align_icp.hip; with_ray: the form
// raycasts the model itself), for the colour ICP to refuse the same
int align_icp_check(tf_volume* v, const float* depth, const float* pose, const float* model_pose, const tf_align_icp_params* p,
                    bool with_iters, bool with_ray);
void reloc_release(tf_volume* v);        // frees tf_reloc.hip's index and forgets its configuration
// The pieces of the device tracker outside tf_devpose.hip, each next to the launches it chains; the caller has checked the
// parameters, nothing is read back.  raycast_posed (tf_ray.hip): tf_raycast_device's launch at the pose in *d_cell.
// track_icp_posed (tf_align_icp.hip): the model raycast at *d_start into the handle's maps and the projective alignment
// from *d_start against them; *d_status is the device word that holds the call's status once its launches are through (-1:
// no pose in the cell).  track_sdf_posed (tf_align.hip): tf_align_frame_device from the 12 floats at d_prev_pose where
// 0 <= *d_prev_status <= TF_ALIGN_MAX_ITERS.  A stage that does not run writes no result: k_track_finish does.
int raycast_posed(tf_volume* v, const tf_device_pose* d_cell, float near_plane, float far_plane, int32_t max_steps,
                  float* d_normal, float* d_vertex);
int track_icp_posed(tf_volume* v, const float* d_depth, const tf_device_pose* d_start, const tf_align_icp_params& p,
                    tf_align_result* d_result, const int32_t** d_status);
// raycast_level (tf_ray.hip): the vertex and normal maps of a pyramid level's camera, at `pose` or at the pose in *d_cell.
int raycast_level(tf_volume* v, const float* pose, const tf_device_pose* d_cell, float near_plane, float far_plane,
                  int32_t max_steps, const AlignCam& cam, float* d_normal, float* d_vertex);
int track_sdf_posed(tf_volume* v, const float* d_depth, const int32_t* d_prev_status, const float* d_prev_pose,
                    const tf_align_params& p, tf_align_result* d_result);
void discard_primed(tf_volume* v);       // the selections made ahead by a streaming call are dropped (tf_capi.cpp)
void devpose_release(tf_volume* v);      // frees tf_devpose.hip's blocks
// the resident model stream (tf_model.hip).  model_pack_enqueue: list, rank, scan and write on the handle's stream, nothing
// read back (the buffers exist and have a capacity); model_stream_sync: the pack, one wait for the control block, the
// buffers grown and the pack repeated on overflow -- ModelState::nv / ni are the counts afterwards; model_release frees all
int model_pack_enqueue(tf_volume* v);
int model_stream_sync(tf_volume* v);
void model_release(tf_volume* v);
void launch_patch_fused(tf_volume* v, const VolumeDev& d, int par, const KfDev& kf, hipStream_t s);
// the same with KfDev::T taken from *d_inv on the device; a block whose gate is off: the launch does nothing
void launch_patch_posed(tf_volume* v, const VolumeDev& d, int par, const KfDev& kf, const PoseInverse* d_inv, hipStream_t s);
inline uint64_t host_pack_id(const int32_t id[3]) {
  return ((uint64_t)((uint32_t)(id[0] + (1 << 20)) & 0x1FFFFFu) << 42) |
         ((uint64_t)((uint32_t)(id[1] + (1 << 20)) & 0x1FFFFFu) << 21) |
         (uint64_t)((uint32_t)(id[2] + (1 << 20)) & 0x1FFFFFu);
}
}  // namespace tf
