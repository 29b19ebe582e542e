/*
 * tf_fusion.h -- C ABI of the MI355X-native voxel-fusion + texture-atlas hot path.
 *
 * This is the drop-in boundary: the reference (THU-luvision/TextureFusion) has no FFI of its
 * own; the "operator API" of the path is the public C++ surface of chisel::Chisel /
 * ChunkManager / Atlas / Patch as called from GCFusion/MobileFusion.{h,cpp}.
 * Each entry point below names the reference interface it stands in for (paths relative to
 * the reference root).  The host-side C++ classes in texturefusion_amd/host/ keep the
 * reference's class/method names and forward to these functions; INTEGRATION.md shows the
 * binding a maintainer adds to the reference tree.
 *
 * Conventions
 *   - plain C, opaque handle, POD arguments only; no exceptions cross the boundary.
 *   - every function returns TF_OK (0) or a negative TF_ERR_* code; tf_last_error() gives the
 *     text of the most recent failure on the calling thread.
 *   - host pointers are borrowed for the duration of the call; outputs are caller-allocated
 *     with a capacity and a count-out.
 *   - one handle = one HIP stream; calls on a handle are serialised by the caller (the
 *     reference drives the path from a single map thread, GCFusion/MobileFusion.cpp:99-112).
 *   - poses are Eigen::Affine3f as 12 floats, row-major 3x4 [R | t] (camera-to-world).
 *   - chunk ids are int32[3]; lists are int32[3*n], order = the reference's list order.
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *     TF_ERR_NO_DEVICE.
 */
#ifndef TF_FUSION_H_
#define TF_FUSION_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define TF_API __attribute__((visibility("default")))
#else
#define TF_API
#endif

#define TF_OK 0
#define TF_ERR_ATLAS_FULL (-1)    /* == Chisel::GeneratePatches' -1 (Structure/Chisel.cpp:170-173) */
#define TF_ERR_INVALID (-2)       /* bad argument / call order */
#define TF_ERR_CAPACITY (-3)      /* chunk pool, list or scratch capacity exceeded */
#define TF_ERR_HIP (-4)           /* HIP runtime error */
#define TF_ERR_NO_DEVICE (-5)     /* no gfx950 device visible */
#define TF_ERR_MISSING_CHUNK (-6) /* list names a chunk that does not exist (chunks.at() would throw) */

typedef struct tf_volume tf_volume;

/* Sizing of the device-resident state (all allocated once, at create). 0 = default. */
typedef struct {
  int32_t device;        /* HIP device ordinal */
  int64_t max_chunks;    /* chunk pool capacity (8 KiB of HBM each); default 1<<20 */
  int64_t max_list;      /* max chunks in one visible-chunk list; default 1<<19 */
  int64_t max_coarse;    /* max 4x4x4 candidate blocks per frame; default 1<<20 */
  int32_t atlas_w;       /* default 13824 (Structure/Atlas.h:29) */
  int32_t atlas_h;       /* default 13824 (Structure/Atlas.h:30) */
  int32_t max_keyframes; /* keyframe image cache slots for the atlas; default 64 */
  /* blocks of the LARGE pool of the mesh store (167 KB each, room for the largest mesh a chunk can have); 0 = default
   * max(256, max_chunks / 64), at most 65535; -1 = none */
  int32_t mesh_overflow_blocks;
  /* device-resident meshes (ChunkManager::allMeshes) live in a store that is allocated ON DEMAND: a chunk-pool slot owns
   * no mesh storage until its chunk first has a mesh with vertices; then it is given a block of mesh_max_vertices /
   * mesh_max_triangles (0 = default 256 / 512: 20.4 KiB; a planar surface through a chunk has 81 / 128) out of
   * mesh_blocks blocks, or -- a mesh has at most 2187 vertices / 2560 triangles (9x9x9x3 edge grid, 512 cells x 5), and
   * the reference emits whatever a chunk produces (Structure/ChunkManager.cpp:856-918) -- a block of the large pool.
   * Once half of a pool has been handed out, a chunk whose mesh comes out empty (Mesh::Clear(), ChunkManager.cpp:254) or
   * outgrows its small block gives the block back and later meshes reuse it: a pool has to hold the meshes that have
   * vertices at one time (plus one generation of turnover), not every mesh there ever was.  Only when the pool a mesh needs
   * is exhausted is the mesh stored empty and reported as TF_ERR_CAPACITY at the next synchronising call. */
  int32_t mesh_max_vertices;
  int32_t mesh_max_triangles;
  /* blocks of the small pool; 0 = default max_chunks: every chunk can own a mesh, as in the reference, whose allMeshes never
   * drops one (ChunkManager.cpp:260-262) -- 20.4 KiB of HBM per pool slot at the default block size.  A caller that knows its
   * scene can take less (about 30 % of the chunks of a scanned room lie on a surface: DESIGN.md s.2); at most max_chunks */
  int64_t mesh_blocks;
} tf_config;

/* Counters of the most recent frame / list (device-side integers, read back on request). */
typedef struct {
  int64_t n_coarse;       /* candidate 4x4x4 blocks tested */
  int64_t n_selected;     /* chunks the reference's selection flags (GetChunkIDsObservedByCamera) */
  int64_t n_updated;      /* list entries whose needsUpdate flag is set */
  int64_t rows_tsdf;      /* 8-voxel rows whose sdf/weight were rewritten by the last integrate */
  int64_t rows_color;     /* 8-voxel rows whose colour was rewritten by the last integrate */
  int64_t n_chunks;       /* chunks alive in the volume */
  int64_t n_slots;        /* pool slots in use (alive + parked) */
  int64_t n_dirty;        /* entries of meshesToUpdate */
  int32_t min_id[3];      /* Chisel::minChunkID */
  int32_t max_id[3];      /* Chisel::maxChunkID */
  int64_t n_listed;       /* = n_selected (kept for layout: a build with depth-tile pruning of the selection subtracted the
                             pruned entries here; variants/r4_experiments.patch) */
} tf_stats;

/* What the textured per-frame unit did for its most recent frame (integers behind the byte counts). */
typedef struct {
  int64_t n_dirty;      /* chunks handed to the mesher */
  int64_t n_meshes;     /* of those, chunks in allMeshes (= patches projected) */
  int64_t n_vertices;   /* vertices of those meshes */
  int64_t n_triangles;
  int64_t roi_pixels;   /* sum of the patches' bounding-box areas */
  int64_t n_patches;    /* patches with an image */
  int64_t n_slots;      /* atlas slots handed out so far */
  int64_t n_exact;      /* dirty chunks whose own voxels were read for the "can it have a vertex" test (the class summaries ruled out the rest) */
  int64_t n_survivors;  /* of those, chunks handed to the marching-cubes kernel */
  int64_t n_surface;    /* of those, chunks in which marching cubes found a cell the surface passes through */
} tf_texture_stats;

/* Per-kernel timings collected with HIP events on the handle's stream (tf_profile_*). */
#define TF_PROF_BBOX 0
#define TF_PROF_SELECT 1
#define TF_PROF_SCAN 2
#define TF_PROF_EMIT 3
#define TF_PROF_INTEGRATE 4
#define TF_PROF_FINALIZE 5
#define TF_PROF_PATCH_PROJECT 6
#define TF_PROF_ATLAS_BLIT 7
#define TF_PROF_MESH 8
#define TF_PROF_DIRTY 9
#define TF_PROF_PATCH_RANK 10
#define TF_PROF_XCHG 11        /* N > 1: pack -> transport -> unpack of one boundary exchange (tf_comm.cpp) */
#define TF_PROF_XCHG_WAIT 12   /* N > 1, overlapped exchange: what the main stream still waits for it behind the interior mesh pass */
#define TF_PROF_COUNT 13
typedef struct {
  double ms[TF_PROF_COUNT];       /* summed elapsed time per kernel */
  int64_t launches[TF_PROF_COUNT];
} tf_profile;

TF_API const char* tf_last_error(void);
TF_API int tf_device_count(void);

/* ---- lifetime / parameters ---------------------------------------------------------
 * Chisel::Chisel(chunkSize, voxelResolution, useColor)   Structure/Chisel.cpp:38-41
 *   (+ ChunkManager ctor, Atlas ctor Structure/Atlas.cpp:32-41).  chunk_dim must be 8x8x8:
 *   the reference kernel hard-codes 512-voxel chunks (ColorVoxel.h:31, Chisel.cpp:81-109). */
TF_API int tf_volume_create(const int32_t chunk_dim[3], float resolution, int use_color,
                            const tf_config* cfg, tf_volume** out);
/* tf_config grows by appended fields and is handed over by pointer: the sized form copies cfg_bytes of it and takes the
 *   defaults (0) for whatever the caller's header did not know.  C / C++ callers get it through the macro below, so a
 *   program built against an older header keeps working against a newer library; tf_volume_create itself stays exported
 *   for bindings that fill the current struct (ctypes, texturefusion_amd/capi.py). */
TF_API int tf_volume_create_sized(const int32_t chunk_dim[3], float resolution, int use_color, const tf_config* cfg,
                                  size_t cfg_bytes, tf_volume** out);
#ifndef TF_NO_SIZED_CREATE
#define tf_volume_create(chunk_dim, resolution, use_color, cfg, out) \
  tf_volume_create_sized((chunk_dim), (resolution), (use_color), (cfg), sizeof(tf_config), (out))
#endif
TF_API int tf_volume_destroy(tf_volume* v);
/* Chisel::Reset   Structure/Chisel.cpp:47-50 */
TF_API int tf_volume_reset(tf_volume* v);
/* Run on an externally owned hipStream_t (e.g. the caller framework's current stream). */
TF_API int tf_set_stream(tf_volume* v, void* hip_stream);
/* PinholeCamera::SetIntrinsics/SetWidth/SetHeight/SetNearPlane/SetFarPlane
 *   3rd_party/open_chisel/camera/PinholeCamera.h:43-57; floats are stored as given and
 *   truncated to int where the reference's int-returning getters do (:46-49). */
TF_API int tf_set_camera(tf_volume* v, float fx, float fy, float cx, float cy, int width,
                         int height, float near_plane, float far_plane);
/* QuadraticTruncator(quadratic, linear, constant, scale)  truncation/QuadraticTruncator.h:33 */
TF_API int tf_set_truncation(tf_volume* v, float quadratic, float linear, float constant,
                             float scale);
/* ConstantWeighter(weight)  weighting/ConstantWeighter.h:34 */
TF_API int tf_set_weight(tf_volume* v, float weight);

/* ---- frame images ------------------------------------------------------------------
 * The reference passes raw cv::Mat data pointers into the path (MobileFusion.cpp:147-149).
 * tf_frame_upload copies host images to HBM; tf_frame_bind_device borrows images that are
 * already device-resident (valid until the next upload/bind).  rgba / quality may be NULL. */
TF_API int tf_frame_upload(tf_volume* v, const float* depth, const uint8_t* rgba,
                           const float* quality);
/* The caller's RGBA staging loop (GCFusion/MobileFusion.cpp:144-163) on the device: rgb = u8[H][W][3]
 * (Frame::rgb), color_valid = u8[H][W] (Frame::colorValidFlag); the path sees
 * rgba = color_valid > 0 ? (r, g, b, 1) : (0, 0, 0, 0). */
TF_API int tf_frame_upload_rgb(tf_volume* v, const float* depth, const uint8_t* rgb,
                               const uint8_t* color_valid, const float* quality);
TF_API int tf_frame_bind_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                const float* d_quality);

/* ---- the path, call by call (the reference's 10-argument flow) ----------------------
 * Chisel::PrepareIntersectChunks   Structure/Chisel.h:103-140
 *   -> chunksIntersecting (out_ids), newChunkFlag (out_new); needsUpdateFlag is all false. */
TF_API int tf_prepare(tf_volume* v, const float pose[12], int32_t* out_ids, uint8_t* out_new,
                      int64_t cap, int64_t* n);
/* Chisel::IntegrateDepthScanColor (10-arg)   Structure/Chisel.h:218-249
 *   integrate_flag 1 = integrate, 0 = de-integrate; keyframe_id / out_quality carry
 *   chunk->observations[keyframeID] (host keeps the map; out_quality may be NULL).
 *   use_color 0 = the call passes colorImage == NULL (depth-only local frames). */
TF_API int tf_integrate(tf_volume* v, const float pose[12], const int32_t* ids, int64_t n,
                        int integrate_flag, int use_color, int use_quality,
                        uint8_t* inout_needs_update, float* out_quality);
/* ---- the keyframe unit (what the product's map thread runs per keyframe) -----------------------------
 * MobileFusion::tsdfFusion (GCFusion/MobileFusion.cpp:274-406) as ONE asynchronous call on device-resident images:
 *   for every MOVED keyframe (GetMapDynamics' keyframesToUpdate, <= 12): RetractObservations (:252-272), then
 *     ReIntegrateKeyframe(flag 0) (:114-221) over the keyframe's stored Frame::validChunks at the OLD poses -- the
 *     keyframe's depth + colour + quality, then its <= 6 local frames depth-only over the same list -- and
 *     ReIntegrateKeyframe(flag 1) at the NEW poses (PrepareIntersectChunks, the same frames, FinalizeIntegrateChunks,
 *     validChunks stored again);
 *   the NEW keyframe group (`fresh`, may be NULL), flag 1;
 *   Chisel::UpdateMeshes over everything marked since the last CompressMeshes (:327);
 *   texture != 0: CompressMeshes, GeneratePatches with the new keyframe as the label of every chunk of chunksToUpdate,
 *     UpdateAtlas (:355-382; pose_inv16 = f32(SE3d.inverse().matrix()) of the new keyframe, Patch.cpp:51).  That labelling
 *     is a shortcut, not the reference's: the reference runs TexMap::view_selection between CompressMeshes and
 *     GeneratePatches (:355-374).  With texture == 0 the unit ends behind UpdateMeshes and the reference's tail follows
 *     with the TexMap resident on the device (tf_texmap_* below): tf_compress_meshes returns chunksToUpdate,
 *     tf_texmap_update / tf_texmap_check_graph / tf_texmap_view_selection keep the chunk graph and the data costs in
 *     HBM, assemble the problem there and assign the solved labels there, tf_generate_patches_selected reads them
 *     there, tf_update_atlas ends the keyframe -- or all of it as ONE call with one host wait, tf_texture_tail_device.
 *     (The host-built path stays: tf_export_* + the host mirror's
 *     TexMap::view_selection + tf_view_select + tf_generate_patches.)  When the resident map exists the unit's
 *     RetractObservations also removes the moved keyframes' data-cost entries (MobileFusion.cpp:261-267).
 * Visible lists, needsUpdate / new flags, every keyframe's validChunks and Chunk::observations (tf_observations_*)
 * stay in HBM; nothing is copied back and the host does not wait.  All images are device pointers (depth f32 16-B
 * aligned; rgba u8[H][W][4] = valid ? (r, g, b, 1) : 0, MobileFusion.cpp:144-163; quality f32 or NULL) that must stay
 * valid until the next synchronising call.  A moved keyframe must have been integrated through this entry point before
 * (its validChunks live in the handle).  tf_keyframe_unit_release frees the per-handle store (also done by
 * tf_volume_reset / tf_volume_destroy). */
typedef struct {
  const float* d_depth;
  const uint8_t* d_rgba;     /* keyframe only; NULL for local frames */
  const float* d_quality;    /* keyframe only; may be NULL */
  float pose[12];            /* row-major [R|t], the pose to integrate with (pose_sophus[0]) */
} tf_unit_frame;
typedef struct {
  int32_t kf_id;             /* Frame::frame_index: key of Chunk::observations, label of its patches */
  int32_t n_local;           /* 0..6 */
  tf_unit_frame keyframe;
  tf_unit_frame local[6];    /* KeyFrameDatabase::corresponding_frames with a refined depth (:189-190) */
  float old_keyframe_pose[12];  /* moved keyframes: the poses of the previous integration (pose_sophus[1]) */
  float old_local_pose[6][12];
} tf_unit_group;
TF_API int tf_keyframe_unit_device(tf_volume* v, const tf_unit_group* fresh, const tf_unit_group* moved, int32_t n_moved,
                                   int32_t texture, const float* pose_inv16);
TF_API int tf_keyframe_unit_release(tf_volume* v);
/* the store of the keyframes' validChunks: out = {capacity, entries in use (top), compactions, stores into an existing
 * region, regions handed out}.  A re-integrated keyframe writes into its region when the list fits, else it gets a new
 * one; the live regions are moved together when the top reaches the capacity.  Synchronises. */
TF_API int tf_keyframe_unit_stats(tf_volume* v, int64_t out[5]);
/* The store has no fixed ceiling: the region table starts with 1024 keyframe slots and doubles when a new keyframe needs
 * one more (the reference sizes its keyframe database for 20 000 frames, main.cpp:81); the arena doubles when the live
 * regions pass three quarters of it (one stream synchronisation + one device copy per doubling).
 * out = {slots of the table, keyframes that own one, doublings so far (table + arena), arena entries}.  Does not synchronise. */
TF_API int tf_keyframe_unit_stats_ex(tf_volume* v, int64_t out[4]);

/* ---- view-selection bookkeeping on the device ------------------------------
 * Chunk::observations (3rd_party/open_chisel/geometry/Chunk.h:171) lives in HBM, keyed by (chunk, keyframe):
 * tf_observations_record   the write of Chisel::IntegrateDepthScanColor (Structure/Chisel.h:244-247) for the list the
 *                          last tf_integrate worked on: observations[keyframe_id] = quality where quality > 0 and the
 *                          chunk's needsUpdateFlag is set (keyframe_id < 0: nothing, as in the reference)
 * tf_observations_retract  MobileFusion::RetractObservations' chunk side (GCFusion/MobileFusion.cpp:252-260):
 *                          observations.erase(keyframe_id) for the listed chunks that exist
 * tf_export_datacost       what TexMap::update_datacost (Structure/TexMap.cpp:64-105) reads, as one table: for chunk i of
 *                          chunksToUpdate out[i * (1 + n_frames) + 0] = observations[frame_index], [1 + j] =
 *                          observations[frames_to_update[j]]; 0 = no observation (recorded qualities are > 0)
 * tf_export_adjacency      the edges TexMap::update_chunkgraph (Structure/TexMap.cpp:50-62) / UniGraph::add_edge_by_node
 *                          (uni_graph.cpp:41-49) add: one record int32[4] = {i, neighbour id} per set Mesh::adj flag of
 *                          chunk ids[i] whose face neighbour (chisel::neighbourhood, ChunkManager.h:55-57) owns a mesh
 *                          (the caller keeps the graph and drops neighbours that are not nodes); order arbitrary */
TF_API int tf_observations_record(tf_volume* v, int32_t keyframe_id);
TF_API int tf_observations_retract(tf_volume* v, int32_t keyframe_id, const int32_t* ids, int64_t n);
TF_API int tf_export_datacost(tf_volume* v, const int32_t* ids, int64_t n, int32_t frame_index,
                              const int32_t* frames_to_update, int32_t n_frames, float* out);
TF_API int tf_export_adjacency(tf_volume* v, const int32_t* ids, int64_t n, int32_t* out_edges, int64_t cap_edges,
                               int64_t* n_edges);
/* TexMap::view_selection's solve (Structure/TexMap.cpp:120-255; the chunksToUpdate overload :257-406 hands over its
 * sub-problem): what the reference gives to mapMAP -- mgraph (:123-137), label_set (:139-155), unaries (:157-180), the
 * Potts pairwise term (:159, :197), the warm start (:208-217) -- and solver.optimize (:199-225) itself.  The objective is
 * mapMAP's (3rd_party/mapmap/source/tree_optimizer.impl.h:158-192, pairwise_potts.impl.h:121-134):
 *   E(x) = sum_i costs_i[x_i] + edge_cost * sum over edges [label_i != label_j]     (edge_cost = adjacent_cost * pairwise_cost)
 * The method is not mapMAP's, and no result of mapMAP is reproduced (it cannot be built here: DESIGN.md s.5): block-
 * coordinate descent over the lattice lines of the chunk graph, each line solved exactly by dynamic programming with the
 * rest held fixed, lines of one axis and one parity class in one launch; a round is the six (axis, class) phases; the
 * solve ends after the first round that changes no label or after max_rounds.  The energy never rises from round to round.
 * All f32 without contraction, ties to the same label and then to the lowest offset: the result is a function of the
 * arguments alone, identical from run to run (tests/mrf_ref.py restates it in numpy).
 *   n_nodes == 0 returns TF_OK and writes nothing.  A node has at most 512 labels (TF_ERR_CAPACITY beyond).
 *   TF_ERR_INVALID (outputs unwritten, no line walked) for: an empty column / col_off not ascending from 0, labels of a
 *   node not strictly ascending or negative, a cost that is not finite, an init offset outside the node's list, a nbr
 *   entry that is not a node, nbr[nbr[i][k]][k ^ 1] != i, ids[nbr[i][k]] != ids[i] + d[k].  One launch in front of the
 *   solve checks all of it; the host form reports the first offending node through tf_last_error.
 * The solve is a pure function of its arguments: it reads and writes no chunk, mesh, atlas texel or observation; the
 * handle supplies the stream and the scratch pool.
 *   out_energy: f64 energies from a fixed-shape reduction, [0] the start labelling, [r] after round r, r <= *out_rounds;
 *   entries behind *out_rounds are left unwritten. */
TF_API int tf_view_select(tf_volume* v, int64_t n_nodes,
    const int32_t* ids,          /* 3 per node: the chunk id */
    const int32_t* nbr,          /* 6 per node, chisel::neighbourhood order: node index across that face, -1 = no edge */
    const int64_t* col_off,      /* n_nodes + 1 */
    const int32_t* labels,       /* nnz, strictly ascending within a node, >= 0 */
    const float*   costs,        /* nnz */
    float edge_cost, const int32_t* init_offsets /* n or NULL = argmin cost, lowest offset */,
    int32_t max_rounds /* 0 = default (32) */,
    int32_t* out_offsets /* n: index into the node's label list, as mapMAP's solution vector */,
    double* out_energy /* NULL or max_rounds + 1: [0] initial, [r] after round r */, int32_t* out_rounds);
/* The same with every array a device pointer (d_init_offsets may be d_out_offsets): enqueues on the handle's stream and
 * does not synchronise.  nnz = col_off[n_nodes]: the host form reads it from its argument, this form cannot without
 * waiting for the device, and its scratch is sized by it (a d_col_off that does not end at nnz is an invalid argument).
 * It cannot return what only the device finds out: when the checking launch finds the arguments invalid (the list
 * above; more than 512 labels) every later launch of the solve returns at once, and d_out_offsets, d_out_energy and
 * d_out_rounds stay unwritten -- a caller that must tell presets d_out_rounds to -1. */
TF_API int tf_view_select_device(tf_volume* v, int64_t n_nodes, const int32_t* d_ids, const int32_t* d_nbr,
                                 const int64_t* d_col_off, int64_t nnz, const int32_t* d_labels, const float* d_costs,
                                 float edge_cost, const int32_t* d_init_offsets, int32_t max_rounds, int32_t* d_out_offsets,
                                 double* d_out_energy, int32_t* d_out_rounds);
/* ---- TexMap resident on the device (Structure/TexMap.{h,cpp}; tf_texmap.hip) -------------------------------------
 * chunkGraph (UniGraph: nodes, edges, labels), dataCost (SparseMat columns) and labelstorage live in HBM per pool slot,
 * allocated by the first tf_texmap_* call (a handle that never makes one keeps its footprint) and freed by
 * tf_volume_reset / tf_volume_destroy.  The reference's `statistic` vector is written and never read
 * (TexMap.cpp:71-75,95) and is not kept.  Every call is asynchronous on the handle's stream unless it says otherwise.
 * tf_texmap_set_keyframes   the kflist of this call: row r <-> kflist[r].keyFrameIndex on the device; its inverse
 *                           frameIndexToKeyframeDB (GCFusion/MobileFusion.cpp:293-296) is kept on the host, where it
 *                           checks the frames an update names (the device keys its costs by frame index).  1 <= n_rows <= 65534 (labels
 *                           are cast to uint16_t, TexMap.cpp:150-151); frame indices >= 0 and distinct.
 * tf_texmap_update          TexMap::update_chunkgraph then update_datacost (TexMap.cpp:50-105) for chunksToUpdate: every
 *                           listed chunk becomes a node (uni_graph.cpp:22-28); then for every listed chunk that owns a
 *                           mesh and every set Mesh::adj flag whose face neighbour is a node the edge is set on both
 *                           ends (uni_graph.cpp:41-49; edges persist until remove_node); observations[frame_index] > 0
 *                           is inserted only where the column has no entry for it (SparseMat::add_value,
 *                           sparse_matrix.cpp:27-36), observations[f] > 0 overwrites for each f of frames_to_update
 *                           (set_value, :38-43), an absent observation removes the entry (:45-50).  The result does not
 *                           depend on the order of ids.  TF_ERR_INVALID for a frame outside the keyframe table.
 * tf_texmap_retract         the data-cost half of MobileFusion::RetractObservations (MobileFusion.cpp:261-267): the entry
 *                           (chunk, keyframe_id) of the listed chunks that exist is removed (a chunk that is no node has
 *                           no column).  tf_keyframe_unit_device does this for its moved keyframes by itself.
 * tf_texmap_remove_wrong_mapping   MobileFusion.cpp:330-342: every mesh in the map whose patch has wrong_mapping loses
 *                           the entry (chunk, patch->frameid); a chunk that is no node is skipped (the reference
 *                           dereferences chunks.find() unchecked).  *n_removed = entries that were there.
 * tf_texmap_check_graph     TexMap::check_graph (TexMap.cpp:107-118): nodes whose mesh has left allMeshes lose their
 *                           edges, on both ends (uni_graph.cpp:89-107), and their column (sparse_matrix.h:67-70); they
 *                           stay nodes.  *n_removed = such nodes.  (n_removed != NULL waits for the count, in both calls.)
 * tf_texmap_view_selection  TexMap::view_selection.  ids == NULL: the full overload (TexMap.cpp:120-255) over every node,
 *                           warm start from the stored labels once a full solve has run (a node without a stored label,
 *                           or whose stored label has left its column, starts at offset 0), the stored labels replaced
 *                           afterwards.  ids != NULL: the sub-problem overload (:257-406) over the listed chunks that
 *                           are nodes; edges to nodes outside it are dropped, cold start, stored labels left alone.
 *                           The problem is assembled on the device as the host mirror's TexMap::solve assembles it
 *                           (labels row + 1 ascending, costs 1.0f - q / column_max in f32, an empty column = the single
 *                           label 0 at cost 1.0f without edges, an edge needs both ends in the problem with non-empty
 *                           columns, edge_cost = 0.5f * 1.0f), solved by tf_view_select_device's launches, and the
 *                           labels are assigned on the device (:227-246): label 0 keeps the chunk's label, or takes
 *                           key_frame_index[n_rows - 2] when the chunk has none and n_rows >= 2; otherwise
 *                           key_frame_index[label - 1].  The host waits ONCE, for the fixed-size control block
 *                           {n_nodes, nnz} that sizes the solver's scratch; no per-chunk data crosses.  max_rounds: 0 =
 *                           32, at most 4096.  out_rounds != NULL (and out_energy, max_rounds + 1 doubles, as in
 *                           tf_view_select) waits for the solve as well; all three outputs may be NULL.
 * tf_texmap_download        mirrors of the listed chunks: is_node, edges (bit k = face k of chisel::neighbourhood),
 *                           label (UniGraph::labels), stored (labelstorage entry, -1 = none at the last full solve) and
 *                           the column as (frame index, quality) pairs in ascending row, packed by col_off[n + 1].
 *                           Any output may be NULL.  Synchronises.
 * tf_texmap_download_problem   the problem assembled last, in tf_view_select's layout (node order = the builder's), with
 *                           the start offsets (-1 each = cold start) and the solved offsets.  Synchronises.
 * tf_texmap_clear           TexMap::clear (TexMap.cpp:408-412), the stored labels included as in the host mirror's; the keyframe table stays. */
TF_API int tf_texmap_set_keyframes(tf_volume* v, const int32_t* key_frame_index, int32_t n_rows);
TF_API int tf_texmap_update(tf_volume* v, const int32_t* ids, int64_t n, int32_t frame_index, const int32_t* frames_to_update,
                            int32_t n_frames);
TF_API int tf_texmap_retract(tf_volume* v, int32_t keyframe_id, const int32_t* ids, int64_t n);
TF_API int tf_texmap_remove_wrong_mapping(tf_volume* v, int64_t* n_removed);
TF_API int tf_texmap_check_graph(tf_volume* v, int64_t* n_removed);
TF_API int tf_texmap_view_selection(tf_volume* v, const int32_t* ids, int64_t n, int32_t max_rounds, double* out_energy,
                                    int32_t* out_rounds, int64_t* out_n_nodes);
TF_API int tf_texmap_download(tf_volume* v, const int32_t* ids, int64_t n, uint8_t* is_node, uint8_t* edges, int32_t* label,
                              int32_t* stored, int64_t* col_off, int32_t* col_frame, float* col_q, int64_t cap_entries);
TF_API int tf_texmap_download_problem(tf_volume* v, int64_t cap_nodes, int64_t cap_nnz, int64_t* n_nodes, int64_t* nnz,
                                      int32_t* ids, int32_t* nbr, int64_t* col_off, int32_t* labels, float* costs,
                                      int32_t* init_offsets, int32_t* offsets);
TF_API int tf_texmap_clear(tf_volume* v);
/* MobileFusion::tsdfFusion's tail (GCFusion/MobileFusion.cpp:330-382) in ONE call, behind tf_keyframe_unit_device(texture = 0)
 *   or tf_update_meshes: the wrong-mapping removal (:330-342; TF_TAIL_WRONG_MAPPING = the caller's integrateKeyframeIndex > 3),
 *   chunksToUpdate (:345-353), CompressMeshes (:355), update_chunkgraph + update_datacost (:356-359), check_graph (:360-361;
 *   TF_TAIL_CHECK_GRAPH = keyframesToUpdate is not empty), view_selection (:362-369; the full overload, or with
 *   TF_TAIL_SUB_PROBLEM the chunksToUpdate overload), GeneratePatches with the labels just assigned (:374) and UpdateAtlas
 *   (:382).  chunksToUpdate never leaves the device: the dirty keys that own a mesh are ranked into ascending chunk id there
 *   (the order the path defines for Atlas::AddPatch) and every stage reads that list.  The host waits ONCE, for the control
 *   block of the solve (which also brings the list's length); nothing else is read back -- an atlas overflow or a label
 *   without a cached keyframe stays in the status word and is reported by the next synchronising call (TF_ERR_ATLAS_FULL /
 *   TF_ERR_INVALID).  Chisel::CompensateColor (:380) is part of the tail with TF_TAIL_COMPENSATE_COLOR: the device path
 *   (tf_compensate_color_device) is enqueued behind UpdateAtlas, the tail still waits once.  CompensateColor reads what
 *   GeneratePatches wrote and nothing UpdateAtlas writes, so that position -- and tf_compensate_color behind a tail without
 *   the flag -- equals the reference's order.  Without the flag CompensateColor is not enqueued.
 *   Chunk ids must lie within +-2^20 per axis (the range of the chunk hash's packed key).
 * tf_texture_tail_list   chunksToUpdate of the last tail, for the caller's DrawMeshes bookkeeping: *n = its length (known
 *   since the tail's wait: out_ids == NULL asks for nothing else and does not synchronise), out_ids = the list in
 *   ascending chunk id (synchronises). */
#define TF_TAIL_WRONG_MAPPING 1u
#define TF_TAIL_CHECK_GRAPH 2u
#define TF_TAIL_SUB_PROBLEM 4u
#define TF_TAIL_COMPENSATE_COLOR 8u
TF_API int tf_texture_tail_device(tf_volume* v, int32_t frame_index, const int32_t* frames_to_update, int32_t n_frames,
                                  uint32_t flags, int32_t max_rounds);
TF_API int tf_texture_tail_list(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n);
/* The local frames of a keyframe group in one visit per chunk (GCFusion/MobileFusion.cpp:187-203: after the keyframe's
 * own IntegrateDepthScanColor, its corresponding frames are integrated depth-only over the SAME chunk list, each with
 * its own pose).  Equivalent, bit for bit, to n_frames successive tf_integrate(use_color = 0) calls with these depth
 * images (device pointers, 16-B aligned) and poses (n_frames x 12 floats); the voxel rows are read and written once
 * instead of n_frames times.  n_frames <= 6 (integrateLocalFrameNum, main.cpp:91). */
TF_API int tf_integrate_depth_group(tf_volume* v, int32_t n_frames, const float* const* d_depth, const float* poses12,
                                    const int32_t* ids, int64_t n, int integrate_flag, uint8_t* inout_needs_update);
/* the same with host depth images (borrowed for the call; staged into a device buffer the handle keeps) */
TF_API int tf_integrate_depth_group_host(tf_volume* v, int32_t n_frames, const float* const* depth, const float* poses12,
                                         const int32_t* ids, int64_t n, int integrate_flag, uint8_t* inout_needs_update);
/* Chisel::FinalizeIntegrateChunks + GarbageCollect   Structure/Chisel.h:184-216,472-477
 *   out_valid receives validChunks (may be NULL). */
TF_API int tf_finalize(tf_volume* v, const int32_t* ids, const uint8_t* needs_update,
                       const uint8_t* is_new, int64_t n, int32_t* out_valid, int64_t* n_valid);

/* ---- the path, fused (the per-frame benchmark unit) ---------------------------------
 * Chisel::IntegrateDepthScanColor (5-arg)   Structure/Chisel.h:453-468, as driven by
 * MobileFusion::IntegrateFrame (GCFusion/MobileFusion.cpp:223-250): prepare -> integrate
 * (flag 1, no keyframe id, no quality) -> finalize on the bound frame.  Asynchronous: no
 * host synchronisation, nothing is copied back.  use_color 0 = rgb.empty() branch. */
TF_API int tf_integrate_frame(tf_volume* v, const float pose[12], int use_color);
/* Same, for a batch of device-resident frames (arrays of n device pointers / n poses). */
TF_API int tf_integrate_frames_device(tf_volume* v, int64_t n_frames, const float* const* d_depth,
                                      const uint8_t* const* d_rgba, const float* poses12);
/* The same for a stream that is fed call by call: the arrays hold n_ahead (0..2) frames more than the
 * n_frames that are integrated; those run through their selection stages (bounding box, visible-chunk
 * list) in this call's launches and the next call, if it starts with exactly these frames (same depth
 * pointer and pose), begins with the voxel update at once -- one launch per frame across calls. */
TF_API int tf_stream_frames_device(tf_volume* v, int64_t n_frames, int64_t n_ahead, const float* const* d_depth,
                                   const uint8_t* const* d_rgba, const float* poses12);
/* The per-frame unit with texturing (BASELINE configs[2]): after frame f is
 * integrated its dirty chunks -- the updated chunks and their six face neighbours, Chisel.h:192-208 -- run
 * through Chisel::UpdateMeshes, CompressMeshes, GeneratePatches with label = frame f and UpdateAtlas
 * (GCFusion/MobileFusion.cpp:327-382 without the host-side view selection), all on the device and without
 * a host synchronisation.  The keyframe of a patch is the frame itself: its RGBA image (alpha ignored) and
 * depth, pose_inv16[f] = f32(SE3d.inverse().matrix()) of its pose; Patch::frameid = first_frame_id + f.
 * New patches take their atlas slots in ascending (x, y, z) chunk-id order within a frame (the reference's
 * order is an unordered_map's).  Chisel::meshesToUpdate collects marks until CompressMeshes clears it: a frame
 * that follows frames integrated WITHOUT this unit (tf_stream_frames_device, tf_integrate ...) inherits their
 * marks and meshes / textures everything they touched as well.
 * IMAGE LIFETIME: with n_ahead == 0 everything that reads the images is on the stream when the call returns.  With
 * n_ahead > 0 the caller declares that it keeps feeding this stream, and the texture stage of the LAST integrated frame
 * (which reads d_rgba[n_frames - 1] and d_depth[n_frames - 1]) is not launched yet: it rides on the next call's first
 * launch.  Those two images must therefore stay valid and unmodified until the next tf_* call on the handle has
 * returned -- a device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) does NOT cover it, tf_sync
 * does (every non-streaming entry point puts the pending stage on the stream first).  A ring of image buffers needs
 * n_ahead + 2 slots. */
TF_API int tf_stream_frames_textured_device(tf_volume* v, int64_t n_frames, int64_t n_ahead,
                                            const float* const* d_depth, const uint8_t* const* d_rgba,
                                            const float* poses12, const float* pose_inv16, int32_t first_frame_id);
/* MobileFusion::IntegrateFrame (GCFusion/MobileFusion.cpp:223-250) as the reference calls it: HOST images in,
 * one call per frame.  The images go through a ring of eight pinned staging / device slots and are uploaded
 * on a second stream, so the H2D of a frame overlaps the kernels of earlier ones and the call returns without
 * synchronising (tf_sync / any state access waits).  Internally the call for frame f launches the integration of
 * frame f - 4 together with the chunk selection of f - 3 and f - 2 (the launch pipeline of the streaming entry points,
 * kept alive across calls; frames f - 1 and f are only staged and copied, so that no launch ever waits for an upload);
 * every other entry point first integrates the frames still in that pipeline, so the deferral is not observable
 * through this API -- but it is LATENCY: a live caller sees frame f in the volume only after four more calls (about
 * 0.4 ms at the bench's rate) or after any synchronising call; the offline loop of main.cpp:272-277 does not care, a
 * caller that needs every frame at once switches the deferral off for its handle with tf_host_frame_set_deferral(v, 0)
 * (integrate in the call that brings the frame; TF_HOST_DEFER=0 in the environment makes that the default of new handles).
 * tf_host_frame_deferral reports both numbers (frames behind, ring slots; v may be NULL).  pose_inv16 != NULL runs the textured unit
 * (tf_stream_frames_textured_device's per-frame work) with Patch::frameid = frame_id; NULL = TSDF only.
 * tf_host_frame_buffers hands out the pinned slot the NEXT call will upload from: a caller that composes its
 * depth / RGBA images there (and passes these pointers) saves the staging copy. */
TF_API int tf_integrate_frame_host(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                   const float* pose_inv16, int32_t frame_id);
/* The same with the colour image as the caller holds it: rgb = u8[H][W][3] (Frame::rgb) and color_valid = u8[H][W]
 * (Frame::colorValidFlag) or NULL (every pixel valid) -- the inputs of the RGBA staging loops the reference runs on the CPU
 * before it calls the path (MobileFusion::IntegrateFrame, GCFusion/MobileFusion.cpp:232-243: alpha = 1 everywhere;
 * :144-163: alpha = colorValid > 0).  7 (or 8) bytes per pixel travel instead of 8 and the loop runs on the device behind
 * the upload.  With tf_host_frame_buffers: rgb at the `rgba` pointer, the flags 3 * W * H bytes behind it. */
TF_API int tf_integrate_frame_host_rgb(tf_volume* v, const float* depth, const uint8_t* rgb, const uint8_t* color_valid,
                                       const float pose[12], const float* pose_inv16, int32_t frame_id);
TF_API int tf_host_frame_buffers(tf_volume* v, float** depth, uint8_t** rgba);
/* A caller that keeps its images in buffers of its own (cv::Mat data, a camera ring) registers them once: the pages are
 * locked in place (hipHostRegister) and host frames that lie inside a registered buffer are uploaded straight out of it --
 * no staging copy, no helper threads -- while the call puts the launches of the frames before on the stream; the call
 * returns when the upload is through, so the buffer is the caller's again on return, as with the staging path.  Registering
 * costs about a millisecond per megabyte: once per buffer, not per frame.  tf_volume_destroy unregisters what is left. */
TF_API int tf_host_register(tf_volume* v, const void* p, int64_t bytes);
TF_API int tf_host_unregister(tf_volume* v, const void* p);
TF_API int tf_host_frame_deferral(tf_volume* v, int32_t* frames_behind, int32_t* ring_slots);
TF_API int tf_host_frame_set_deferral(tf_volume* v, int on);
/* A caller with a RING of registered frame buffers need not wait for every upload: tf_host_frame_set_async(v, 1) lets a call
 * out of registered buffers return as soon as its upload is queued (the reference's contract -- "the buffer is mine again
 * when the call returns", MobileFusion.cpp:249 -- is then the caller's to keep); tf_host_frame_fence(v) returns when every
 * upload queued so far is through, i.e. every buffer handed over so far may be written again.  The upload of frame f then
 * overlaps the call for f + 1: a TSDF-only stream runs at the link's rate (2.46 MB per 640x480 frame at 46 GB/s = 53 us,
 * tools/h2d_probe.py) instead of upload + call time.  Default off. */
TF_API int tf_host_frame_set_async(tf_volume* v, int on);
TF_API int tf_host_frame_fence(tf_volume* v);
/* Where the host side of tf_integrate_frame_host(_rgb) spends its time, summed since create / the last reset:
 * out[0] = calls that put a frame's launches on the stream, out[1..5] = microseconds spent waiting for the device to free
 * a staging slot (back-pressure: the device is the bound), waiting for the slot's previous upload, in the staging copy, in
 * the upload enqueue, in the kernel launches; out[6] = launches that had to wait in the stream for an upload. */
TF_API int tf_host_frame_times(tf_volume* v, double out[7], int reset);
/* The texturing half of the per-frame unit on its own, for the frame integrated last (its images still bound):
 * UpdateMeshes -> CompressMeshes -> GeneratePatches(label = frame_id) -> UpdateAtlas over that frame's dirty
 * chunks.  tf_stream_frames_textured_device == per frame: voxel update, then this.  A multi-GPU host that
 * brings its own transport calls tf_boundary_pack_block / its all-gather / tf_boundary_unpack_blocks(join_dirty)
 * in between. */
TF_API int tf_texture_frame_device(tf_volume* v, const float pose_inv16[16], int32_t frame_id);
/* The same in two halves around the caller's own boundary exchange, so that the exchange overlaps work: phase 1 builds the
 * frame's dirty set and meshes its INTERIOR chunks (those whose 27-chunk neighbourhood this rank owns: nothing they read
 * comes from another rank); phase 2 meshes the boundary chunks and everything the arriving ghosts added, and leaves the
 * patch stage pending as tf_texture_frame_device does.  Order for the caller's transport:
 *   - tf_boundary_unpack_*(join_dirty) must run BEHIND phase 1 and ahead of phase 2: phase 1's filter walks the flat work
 *     list of the frame's parity, the list join_dirty appends to (the library's own overlapped exchange hands its interior
 *     pass an empty flat list instead; this entry point does not).  The tf_boundary_unpack_* entry points launch on the
 *     handle's stream, so calling them after phase 1 gives that order;
 *   - what may overlap phase 1 is the PACK and the TRANSPORT: issue tf_boundary_pack_* before phase 1 (it reads voxels the
 *     frame's update has finished writing and nothing phase 1 writes) and run the transport on the caller's own stream or
 *     thread while phase 1's launches execute; a pack issued after phase 1 sits behind it on the handle's stream and
 *     overlaps nothing.
 * Results equal the one-call form bit for bit.  (With tf_comm_exchange_every_frame the library does this itself, pack /
 * send / receive / unpack on a second stream next to the interior pass: tf_comm_exchange_overlap(v, 0) switches that off.) */
TF_API int tf_texture_frame_device_phase(tf_volume* v, const float pose_inv16[16], int32_t frame_id, int phase);
TF_API int tf_comm_exchange_overlap(tf_volume* v, int on);
TF_API int tf_sync(tf_volume* v);

/* ---- state access (host mirrors of Chunk::voxels / colors, ChunkManager queries) -----
 * ChunkManager::HasChunk   Structure/ChunkManager.h:133-135 */
TF_API int tf_has_chunk(tf_volume* v, const int32_t id[3], int* out);
/* Chunk::voxels.sdf / .weight (DistVoxel.h:102-103), Chunk::colors.colorData
 *   (ColorVoxel.h:66) in the reference's layouts: sdf[512], weight[512], color[512*4]. */
TF_API int tf_chunk_download(tf_volume* v, const int32_t id[3], float* sdf, float* weight,
                             uint16_t* color);
TF_API int tf_chunks_download(tf_volume* v, const int32_t* ids, int64_t n, float* sdf,
                              float* weight, uint16_t* color);
/* creates the chunk if needed (ChunkManager::CreateChunk, ChunkManager.cpp:266-270) */
TF_API int tf_chunk_upload(tf_volume* v, const int32_t id[3], const float* sdf,
                           const float* weight, const uint16_t* color);
/* ChunkManager::GetChunks() keys */
TF_API int tf_list_chunks(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n);
/* Chisel::meshesToUpdate (Structure/Chisel.h:489): keys with value true */
TF_API int tf_list_dirty(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n);
TF_API int tf_clear_dirty(tf_volume* v);
TF_API int tf_get_stats(tf_volume* v, tf_stats* out);
TF_API int tf_get_texture_stats(tf_volume* v, tf_texture_stats* out);

/* ---- reading the volume back (tf_ray.hip) -----------------------------------------------
 * These calls only read the volume: no voxel, hash entry, dirty mark, mesh-filter summary, neighbour-table word or
 * statistic changes.  A chunk that is not alive counts as absent (as in tf_has_chunk).  A handle with an active
 * communicator (tf_comm_init) answers from its own chunks and the ghosts it holds (the raycast, the point queries,
 * GetDistanceFromSurface and RefineFrameInVoxel alike); there is no multi-rank raycast.
 *
 * Batched point queries: n world points xyz (f32[3n]); want_mask selects the outputs, flags[i] gets one bit per
 * output that is valid at point i (an invalid output is written as 0):
 *   bit 0  sdf[n]      ChunkManager::GetSDF (Structure/ChunkManager.cpp:1168-1185): the voxel that contains the point,
 *                      valid if its chunk exists and weight > 1e-12
 *   bit 1  weight[n]   ChunkManager::GetWeight (:1151-1166): the same voxel, valid whenever its chunk exists
 *   bit 2  grad3[3n]   ChunkManager::GetSDFAndGradient (:1043-1141, live branch): point snapped to its voxel centre,
 *                      (x+ - x-, y+ - y-, z+ - z-) of the six face neighbours (across a chunk face: the adjacent chunk,
 *                      voxelNeighborIndex :108-140), unnormalised; invalid if a chunk is missing or a value is >= 1
 *                      (GetNeighborSDF, ChunkManager.h:755-788)
 *   bit 3  sdf_tri[n]  trilinear SDF over the 8 voxel centres around the point (order of operations: tf_ray.hip),
 *                      valid if all 8 exist with weight > 0
 *   bit 4  rgb3[3n]    trilinear colour of the per-voxel means R / count ... (ColorVoxel.h:44-55), rounded half up to
 *                      u8, valid if all 8 corners have count > 0
 * tf_query_points takes host arrays, is ordered after every call already issued on the handle and returns when the
 * results are there; _device takes device pointers and is asynchronous on the handle's stream. */
TF_API int tf_query_points(tf_volume* v, const float* xyz, int64_t n, uint32_t want_mask, float* sdf, float* weight,
                           float* grad3, float* sdf_tri, uint8_t* rgb3, uint32_t* flags);
TF_API int tf_query_points_device(tf_volume* v, const float* d_xyz, int64_t n, uint32_t want_mask, float* d_sdf,
                                  float* d_weight, float* d_grad3, float* d_sdf_tri, uint8_t* d_rgb3, uint32_t* d_flags);
/* Model view from a pose (what frame-to-model tracking reads; the reference renders its meshes with GL instead,
 * Chisel::DrawMeshes + MobileFusion.h:404-446).  pose: camera-to-world 3x4 as in tf_integrate.  The ray of pixel (x, y)
 * runs through camera point ((x - cx - 0.5) / fx, (y - cy - 0.5) / fy, 1) with the int-truncated intrinsics of
 * tf_set_camera (the integrator's projection, so a surface renders back at the depth it was integrated from) or of
 * tf_raycast_camera.  March: whole chunks skipped where the chunk is absent, one voxel while the trilinear SDF is
 * invalid, max(voxel, 0.75 * sdf) where it is valid; a hit is the first + -> - crossing, t refined linearly between the
 * two samples; a - -> + crossing, t > far_plane or max_steps samples end the ray as a miss.  Outputs (NULL = not
 * written): depth f32[H][W] camera-frame z, 0 = miss; normal f32 planar [3][H][W] world-frame unit normal from the
 * trilinear SDF's central differences (one-sided against the hit on an axis where one tap is invalid; 0 where both are, or on a miss); rgba u8[H][W][4] the bit-4 colour,
 * a = 255 on a hit, 0 on a miss; vertex f32 planar [3][H][W] world hit point.  Needs 0 <= near < far, max_steps > 0.
 * tf_raycast: host outputs, synchronous; _device: device outputs, asynchronous on the handle's stream. */
TF_API int tf_raycast(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t max_steps,
                      float* depth, float* normal, uint8_t* rgba, float* vertex);
TF_API int tf_raycast_device(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t max_steps,
                             float* d_depth, float* d_normal, uint8_t* d_rgba, float* d_vertex);
/* camera of the raycaster, the renderer and the aligner only (intrinsics truncated to int like tf_set_camera's; any width up to 32768); width = height
 * = 0 goes back to the camera of tf_set_camera.  fx, fy >= 1; fx, fy, cx, cy finite and of magnitude below 2^31.  Every
 * output of tf_raycast(_device) holds the W x H of the camera active at the call. */
TF_API int tf_raycast_camera(tf_volume* v, float fx, float fy, float cx, float cy, int width, int height);
/* Chisel::GetDistanceFromSurface (Structure/Chisel.h:251-342) for n world points xyz (f32[3n]): the SDF averaged over
 * the 8 voxels around p - res / 2 with trilinear weights times voxel weight (floor / ceil corners as the reference
 * forms them, absent chunks skipped; order of operations: tf_ray.hip).  dist[i] = sum(sdf sw w) / sum(sw w) and
 * tsdf_weight[i] = sum(w sw) / sum(sw w), both left as accumulated (0 where no corner exists) when sum(sw w) <= 0.
 * A corner whose voxel coordinate is not finite or beyond +-(2^23 - 1) is absent.  n = 0 is a no-op. */
TF_API int tf_distance_from_surface(tf_volume* v, const float* xyz, int64_t n, float* dist, float* tsdf_weight);
TF_API int tf_distance_from_surface_device(tf_volume* v, const float* d_xyz, int64_t n, float* d_dist,
                                           float* d_tsdf_weight);
/* Chisel::RefineFrameInVoxel (Structure/Chisel.h:377-451): depth (W x H of tf_set_camera) refined in place, weight
 * written; pixels the reference skips keep both values.  pose: camera-to-world 3x4 as in tf_integrate.
 * A pixel with depth < 0.05 or > 3 is skipped.  Otherwise, along the ray ((j - cx) / fx, (i - cy) / fy, 1) of the
 * int-truncated intrinsics, depth += GetDistanceFromSurface(vertex(depth)) six times; weight = the sixth call's
 * tsdf_weight; then depth and weight are set to 0 where |sixth distance| > 5e-3, where depth is outside
 * [near, far] of the camera, or where |depth - initial depth| > 0.1 (in that order, on the value written so far).
 * A NaN depth stays NaN with weight 0.  tf_refine_frame_in_voxel: host images, synchronous; _device: device images,
 * asynchronous on the handle's stream (a device depth image refined in place can go on to tf_frame_bind_device /
 * tf_integrate_frames_device with no host round trip). */
TF_API int tf_refine_frame_in_voxel(tf_volume* v, float* depth, float* weight, const float pose[12]);
TF_API int tf_refine_frame_in_voxel_device(tf_volume* v, float* d_depth, float* d_weight, const float pose[12]);

/* ---- frame-to-model alignment (tf_align.hip) ---------------------------------------------
 * Given a depth image (W x H and intrinsics of tf_raycast_camera if one is set, else of tf_set_camera) and an approximate camera-to-world pose, find the pose at which the frame
 * lies on the fused surface: Gauss-Newton on the trilinear SDF at the back-projected pixels (the step the reference
 * leaves commented out at GCFusion/MobileFusion.cpp:322; the method is this library's own, its order of operations is
 * fixed in tf_align.hip and restated in tests/align_ref.py).  Read-only, as the calls above.
 *
 * Level l samples the pixels with x % stride[l] == 0 && y % stride[l] == 0 and takes up to iters[l] steps.  A sampled
 * pixel whose depth z is finite and in [min_depth, max_depth] gives the camera point ((x - cx - 0.5) / fx * z,
 * (y - cy - 0.5) / fy * z, z) (int-truncated intrinsics: the raycaster's ray), the world point pw = t + R pc, the
 * trilinear SDF s at pw and at pw +- one voxel along each axis.  The pixel is valid when all seven samples are and
 * |s| <= max_residual.  Residual r = s, gradient g by central differences, Jacobian [g, (R pc) x g] of a twist (v, w)
 * about the camera centre (R <- exp([w]x) R, t <- t + v), weight 1 where huber == 0 or |r| <= huber, else huber / |r|.
 * One evaluation sums A = sum w J J^T, b = sum w J r, sum r^2, sum w r^2 in f64 in an order that depends on (W, H, stride)
 * alone; a step solves (A + damping diag(A)) xi = -b by Cholesky and updates the pose (carried in f64).
 * Stops: n_valid < min_valid -> TF_ALIGN_TOO_FEW; a pivot <= 1e-12 * the largest diagonal entry -> TF_ALIGN_SINGULAR
 * (a plane alone); on either the pose of that evaluation is the result and nothing further is sampled.  A level ends
 * early when |v| < eps_t && |w| < eps_r; at the last level that is TF_ALIGN_CONVERGED, otherwise the call ends as
 * TF_ALIGN_MAX_ITERS.  After the last step one closing evaluation records the final sums and makes no update.
 * The status is a field of the result, not the return value: a call that stops returns TF_OK. */
#define TF_ALIGN_CONVERGED 0
#define TF_ALIGN_MAX_ITERS 1
#define TF_ALIGN_TOO_FEW 2
#define TF_ALIGN_SINGULAR 3
#define TF_ALIGN_MAX_EVALUATIONS 65 /* 64 steps and the closing evaluation */
typedef struct tf_align_params {
  int32_t n_levels;               /* 1..4 */
  int32_t stride[4], iters[4];    /* stride >= 1; iters >= 0, sum of iters <= 64 */
  float min_depth, max_depth, max_residual, huber, damping, eps_t, eps_r;
  int32_t min_valid;
} tf_align_params;
typedef struct tf_align_result {
  int32_t status, evaluations, n_sampled, n_valid_first, n_valid_last; /* n_sampled: of the last evaluation */
  float rms_first, rms_last;      /* sqrt(sum r^2 / n_valid), unweighted; 0 where n_valid == 0 */
  float pose[12];
} tf_align_result;
typedef struct tf_align_iter {    /* one per evaluation, closing one included */
  int32_t level, stride, n_sampled, n_valid;
  double sum_r2, sum_wr2, A[21], b[6], xi[6], pose[12]; /* A: upper entries row by row; xi: the step taken (0: none);
                                                           pose: the one the sums were taken at */
} tf_align_iter;
/* strides {4, 2, 1}, iters {4, 3, 2}, depth in [0.05, 5], max_residual 0.03, huber 0.01, damping 0, eps 1e-5 / 1e-5,
 * min_valid 100 */
TF_API int tf_align_default_params(tf_align_params* out);
/* TF_ERR_INVALID (nothing launched) for n_levels outside 1..4, a stride < 1, a negative iters entry or a sum above 64,
 * a non-finite parameter or pose entry, min_depth > max_depth, negative huber / damping / eps_t / eps_r, no camera.
 * tf_align_frame: host image, synchronous (it waits once, for the result).  _device: device image and device result,
 * asynchronous on the handle's stream: every launch of the call is enqueued up front, a launch behind a stop returns at
 * once, nothing is read back. */
TF_API int tf_align_frame(tf_volume* v, const float* depth, const float pose[12], const tf_align_params* params,
                          tf_align_result* result);
TF_API int tf_align_frame_device(tf_volume* v, const float* d_depth, const float pose[12], const tf_align_params* params,
                                 tf_align_result* d_result);
/* the records of the last tf_align_frame(_device) call of this handle (waits for it): up to cap of them to out (may be
 * NULL with cap 0), *n = how many there are.  A of a record is the information matrix of the pose at that evaluation. */
TF_API int tf_align_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n);
/* The residual map of one evaluation at stride[0] (iters are not read): r f32[H][W], grad3 f32 planar [3][H][W],
 * flags u32[H][W]; any may be NULL.  flags: bit 0 depth in range, bit 1 centre sample valid, bit 2 all six taps valid,
 * bit 3 |s| <= max_residual; each bit is set only where the ones below it are, a pixel is valid when flags == 15.
 * r = s where bits 0 and 1 are set, else 0; grad where bits 0 to 2 are set, else 0; pixels not sampled get 0 everywhere. */
TF_API int tf_align_residuals(tf_volume* v, const float* depth, const float pose[12], const tf_align_params* params,
                              float* r, float* grad3, uint32_t* flags);
TF_API int tf_align_residuals_device(tf_volume* v, const float* d_depth, const float pose[12],
                                     const tf_align_params* params, float* d_r, float* d_grad3, uint32_t* d_flags);

/* ---- alignment by colour as well as depth (tf_align_color.hip) -----------------------------
 * tf_align_frame with a photometric row beside each geometric one, so that the pose is also held inside a surface (a
 * wall, a floor, a table top: there the geometric call ends TF_ALIGN_SINGULAR or at a pose that depends on its start).
 * rgba is the frame's u8[H][W][4] image as the integrator takes it (alpha = colour valid), of the same camera as depth.
 * The geometric row, its flag bits 0 to 3 and its sums are tf_align_frame's.  The model's intensity at a point is the
 * trilinear mean of the eight corners' (0.299 R + 0.587 G + 0.114 B) / n / 255 (n: the voxel's colour count; valid where
 * every corner has n > 0), the frame's the same combination of the pixel.  rc = L(pw) - Lf, its gradient gc by central
 * differences over one voxel, Jacobian [gc, (R pc) x gc], Huber weight with huber_photo.  Flag bit 4: bits 0..3 set,
 * alpha != 0 and L(pw) valid; bit 5: all six taps' intensities valid; bit 6: |rc| <= max_photo_residual; each bit is set only
 * where the lower ones are, a pixel is photometrically valid when flags == 127 and geometrically when (flags & 15) == 15.
 * A step solves (A + photo_weight^2 A_c + damping diag) xi = -(b + photo_weight^2 b_c); everything else -- levels, stops
 * (TF_ALIGN_TOO_FEW goes by the geometric n_valid), the closing evaluation, the status -- is tf_align_frame's.  With
 * photo_weight == 0 or on a volume without colour the pose, the status and the geometric sums are tf_align_frame's bit
 * for bit.  No image gradients, no blurred pyramids (exposure: tf_align_set_exposure).  Read-only; its state and log are its own:
 * tf_align_log keeps meaning the last tf_align_frame call. */
typedef struct tf_align_color_params {
  tf_align_params geo;
  float photo_weight, max_photo_residual, huber_photo; /* intensities in [0, 1]; all >= 0 */
} tf_align_color_params;
typedef struct tf_align_color_result {
  tf_align_result geo;
  int32_t n_photo_first, n_photo_last;     /* photometrically valid pixels of the first / last evaluation */
  float rms_photo_first, rms_photo_last;   /* sqrt(sum rc^2 / n_photo), unweighted; 0 where n_photo == 0 */
} tf_align_color_result;
typedef struct tf_align_color_iter {       /* one per evaluation, closing one included */
  tf_align_iter geo;                       /* geo.A, geo.b: the geometric sums alone; geo.xi: the step of the combined system */
  int32_t n_photo, pad;
  double sum_rc2, sum_wrc2, Ac[21], bc[6];
} tf_align_color_iter;
/* geo = tf_align_default_params', photo_weight 0.1, max_photo_residual 0.25, huber_photo 0.05 */
TF_API int tf_align_color_default_params(tf_align_color_params* out);
/* TF_ERR_INVALID (nothing launched) for what tf_align_frame rejects and for a negative or non-finite photo_weight,
 * max_photo_residual or huber_photo.  tf_align_frame_color: host images, synchronous (it waits once, for the result).
 * _device: device images (rgba 4-byte aligned) and device result, asynchronous on the handle's stream. */
TF_API int tf_align_frame_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                const tf_align_color_params* params, tf_align_color_result* result);
TF_API int tf_align_frame_color_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                       const tf_align_color_params* params, tf_align_color_result* d_result);
/* the records of the last tf_align_frame_color(_device) call of this handle (waits for it), as tf_align_log */
TF_API int tf_align_color_log(tf_volume* v, tf_align_color_iter* out, int64_t cap, int64_t* n);
/* The maps of one evaluation at geo.stride[0]: r, grad3 and flags as tf_align_residuals', rc f32[H][W] (where bit 4 is
 * set, else 0) and gradc3 f32 planar [3][H][W] (where bit 5 is set, else 0); any may be NULL; pixels not sampled get 0. */
TF_API int tf_align_color_residuals(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                    const tf_align_color_params* params, float* r, float* grad3, float* rc, float* gradc3,
                                    uint32_t* flags);
TF_API int tf_align_color_residuals_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                           const tf_align_color_params* params, float* d_r, float* d_grad3, float* d_rc,
                                           float* d_gradc3, uint32_t* d_flags);

/* ---- a keyframe group aligned in one call (tf_align_group.hip) -----------------------------
 * OptimizeKeyframeVoxelDomain (GCFusion/MobileFusion.cpp:322) for the unit ReIntegrateKeyframe integrates: a keyframe and
 * its up to six local frames, all of the readers' camera.  body[k] names the rigid body frame k belongs to (NULL: all
 * frames are body 0); bodies are numbered by first appearance (body[0] == 0, body[k] <= 1 + max(body[0..k-1])) and a
 * body's anchor is its first frame.  Every body has its own 6 x 6 system, its own twist per step and its own stops, by
 * tf_align_frame's rules exactly (min_valid goes by the body's total n_valid); one body stopping does not stop the others.
 * A frame's rows are tf_align_frame's, except that the twist of a body is taken about its anchor's camera centre: a
 * later frame's Jacobian is [g, ((t_k - t_anchor) + R_k pc) x g].  A body's sums are its frames' sums (each formed as
 * tf_align_frame forms them) added in ascending frame order; a step moves every frame of the body by the same rigid
 * motion, R_k <- E R_k, t_k <- c + E (t_k - c) + v with c the anchor's centre before the step.  A body of one frame has
 * tf_align_frame's result and log bit for bit.  A call is 1 + 2 launches per evaluation, as tf_align_frame, whatever
 * the number of frames.  Read-only; its state and log are its own: tf_align_log and tf_align_color_log keep their meaning.
 * Not here: a photometric row, more than seven frames, frames of different cameras, multi-rank alignment.
 * TF_ERR_INVALID (nothing launched, the result untouched) for what tf_align_frame rejects, for any frame; n_frames
 * outside 1..7; a null image pointer; a body array that breaks the numbering rule; a null result. */
#define TF_ALIGN_GROUP_MAX_FRAMES 7   /* a keyframe and six local frames: tf_unit_group */
typedef struct tf_align_group_result {
  int32_t n_frames, n_bodies;
  tf_align_result body[TF_ALIGN_GROUP_MAX_FRAMES];   /* one per body; .pose = the body's anchor frame; n_sampled, n_valid_*: summed over its frames */
  float pose[TF_ALIGN_GROUP_MAX_FRAMES][12];         /* every frame's pose at the end */
  int32_t frame_valid_first[TF_ALIGN_GROUP_MAX_FRAMES], frame_valid_last[TF_ALIGN_GROUP_MAX_FRAMES];  /* per frame: valid pixels of its body's first / last evaluation */
} tf_align_group_result;
/* d_depth / depth: host arrays of n_frames image pointers (device images for _device, host images for the other form);
 * poses12: n_frames x 12 floats.  _device: device result, asynchronous on the handle's stream, every launch enqueued up
 * front, nothing read back.  tf_align_group stages the images through the handle's scratch pool and waits once, for the
 * result.  Entries of the result past n_bodies / n_frames are zero. */
TF_API int tf_align_group_device(tf_volume* v, int32_t n_frames, const float* const* d_depth, const float* poses12,
                                 const int32_t* body, const tf_align_params* params, tf_align_group_result* d_result);
TF_API int tf_align_group(tf_volume* v, int32_t n_frames, const float* const* depth, const float* poses12,
                          const int32_t* body, const tf_align_params* params, tf_align_group_result* result);
/* the records of body `body` (0..6) of the handle's last group call (waits for it), as tf_align_log; a record's pose is
 * the anchor's; a body that call did not have has no records */
TF_API int tf_align_group_log(tf_volume* v, int32_t body, tf_align_iter* out, int64_t cap, int64_t* n);
/* The same for the struct tf_keyframe_unit_device takes: frame 0 is group->keyframe, frames 1 + i are group->local[i]
 * (i < n_local), the images are the struct's device depth pointers.  rigid != 0: one body; otherwise every frame is its
 * own.  Waits once, then writes the aligned pose into the pose field of every frame whose body ended with status <=
 * TF_ALIGN_MAX_ITERS; the other frames and old_* stay as they are. */
TF_API int tf_align_unit_group(tf_volume* v, tf_unit_group* group, int rigid, const tf_align_params* params,
                               tf_align_group_result* result);

/* ---- tracking a frame from far off: projective ICP against the raycast model (tf_align_icp.hip) ---
 * tf_align_frame samples the SDF at the frame's points, so it only captures a start within the truncation band (a couple
 * of centimetres).  This is KinectFusion's projective point-to-plane ICP against the model's vertex and normal maps, as
 * tf_raycast_device writes them (f32 planar [3][H][W], world frame, normal 0 on a miss), of the same camera as the depth
 * image and rendered from model_pose: a pixel needs only to project onto a model pixel whose point lies within
 * max_distance.  Per sampled pixel: pw as tf_align_frame's (flag bit 0: depth in range); pm = Rm^T (pw - tm), the model
 * pixel (u, v) = floor(f * pm.xy / pm.z + (c + 0.5) + 0.5), the one whose raycast ray is the nearest (bit 1: pm.z > min_depth
 * and (u, v) inside the image); vm, nm the maps there (bit 2: |nm|^2 > 0.5, a hit); e = pw - vm, r = nm . e (bit 3: |e|^2 <= max_distance^2
 * and |r| <= geo.max_residual).  Each bit is set only where the lower ones are; a pixel is valid when flags == 15.
 * Jacobian [nm, (R pc) x nm]: tf_align_frame's twist about the camera centre.  Huber weight, sums and their order, the
 * solve, the pose update, levels, stops, statuses, the closing evaluation, tf_align_result and tf_align_iter are
 * tf_align_frame's; a plane alone still ends TF_ALIGN_SINGULAR (tf_align_frame_icp_color below holds it).  The order of operations is fixed in tf_align_icp.hip
 * and restated in tests/align_icp_ref.py.  The maps and the model pose do not change during a call; re-rendering between
 * levels is the caller's choice, through a second call.  A call is 1 + 2 launches per evaluation, all enqueued up front.
 * Read-only; its state and log are its own: tf_align_log, tf_align_color_log and tf_align_group_log keep their meaning.
 * A normal-compatibility gate from the frame's own normals is a setting of the handle: the section below tf_track_frame.
 * So is a depth pyramid for the coarse levels (the section after that one); without it a level samples by stride alone.
 * A photometric row beside the geometric one is a call of its own: tf_align_frame_icp_color, below the pyramid's section.
 * Not here: a group form, multi-rank. */
typedef struct tf_align_icp_params {
  tf_align_params geo;     /* levels, depth range, huber, damping, eps, min_valid; max_residual gates |r| */
  float max_distance;      /* gate on |pw - vm| */
  float ray_near, ray_far; int32_t ray_max_steps;   /* for the forms that raycast themselves */
} tf_align_icp_params;
typedef struct tf_track_result {
  tf_align_result icp, sdf;   /* sdf.status == -1 (the rest 0): the SDF stage was not run */
  int32_t stage;              /* 0 none usable, 1 icp only, 2 sdf */
  float pose[12];
} tf_track_result;
/* strides {4, 2, 1}, iters {6, 4, 3}, depth in [0.05, 5], max_distance 0.15, max_residual 0.15 (not binding: |r| <= |e|),
 * huber 0.02, damping 0, eps 1e-5 / 1e-5, min_valid 100, ray 0.05 / 5 / 1024 */
TF_API int tf_align_icp_default_params(tf_align_icp_params* out);
/* TF_ERR_INVALID (nothing launched, the result untouched) for what tf_align_frame rejects; a negative or non-finite
 * max_distance; a null map or result pointer; a non-finite model pose entry; in the forms that raycast themselves, ray
 * parameters tf_raycast rejects.
 * _device: everything in device memory (model_pose on the host, not NULL), asynchronous on the handle's stream, nothing
 * read back.  tf_align_frame_icp: host depth image staged through the scratch pool; the model is raycast at model_pose
 * (NULL: at pose) by tf_raycast_device's launch into maps the handle owns; it waits once, for the result. */
TF_API int tf_align_frame_icp_device(tf_volume* v, const float* d_depth, const float pose[12], const float* d_model_vertex,
                                     const float* d_model_normal, const float model_pose[12],
                                     const tf_align_icp_params* params, tf_align_result* d_result);
TF_API int tf_align_frame_icp(tf_volume* v, const float* depth, const float pose[12], const float* model_pose,
                              const tf_align_icp_params* params, tf_align_result* result);
/* the records of the last tf_align_frame_icp(_device) or tf_track_frame call of this handle (waits for it), as tf_align_log */
TF_API int tf_align_icp_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n);
/* The maps of one evaluation at geo.stride[0] (iters are not read): r f32[H][W] (where bits 0 to 2 are set, else 0), flags
 * u32[H][W], assoc i32[H][W] = v * W + u of the associated model pixel where bit 1 is set, else -1; any may be NULL;
 * pixels not sampled get 0, 0 and -1.  The host form takes host maps, or raycasts the model at model_pose (NULL: at pose)
 * where model_vertex and model_normal are both NULL. */
TF_API int tf_align_icp_residuals(tf_volume* v, const float* depth, const float pose[12], const float* model_vertex,
                                  const float* model_normal, const float* model_pose, const tf_align_icp_params* params,
                                  float* r, uint32_t* flags, int32_t* assoc);
TF_API int tf_align_icp_residuals_device(tf_volume* v, const float* d_depth, const float pose[12],
                                         const float* d_model_vertex, const float* d_model_normal,
                                         const float model_pose[12], const tf_align_icp_params* params, float* d_r,
                                         uint32_t* d_flags, int32_t* d_assoc);
/* The coarse-to-fine tracker in one call: tf_align_frame_icp with the model raycast at the start pose; where that ends
 * with status <= TF_ALIGN_MAX_ITERS, tf_align_frame from the ICP's pose.  out->pose is the SDF stage's pose where its
 * status <= TF_ALIGN_MAX_ITERS (stage 2), otherwise the ICP's where the ICP's was (stage 1), otherwise the caller's
 * (stage 0).  It waits twice, once per stage; tf_track_frame_device below chains the stages on the device, from a pose in
 * device memory, and waits for nothing.  TF_ERR_INVALID (nothing launched, out untouched) for what either stage rejects. */
TF_API int tf_track_frame(tf_volume* v, const float* depth, const float pose[12], const tf_align_icp_params* icp_params,
                          const tf_align_params* sdf_params, tf_track_result* out);

/* ---- the projective ICP gated by frame normals (tf_align_icp_gate.hip) --------------------------
 * KinectFusion's third rejection test.  Without it a pixel of one wall that projects onto the model's image of another
 * wall is a valid pair whenever the two points lie within max_distance: at every concave or convex edge.  The gate is a
 * setting of the handle, off in a new handle and off again after tf_volume_reset.  Every call that runs the projective ICP
 * reads it: tf_align_frame_icp(_device), tf_align_icp_residuals(_device), tf_track_frame, tf_track_frame_device,
 * tf_track_integrate_device, tf_track_texture_device, tf_relocalise.
 * The frame normal of a sampled pixel (x, y) at the level's stride s, depth z0 in range (bit 0), from its neighbours
 * L = (x - s, y), R = (x + s, y), U = (x, y - s), D = (x, y + s): it exists iff all four lie inside the image, each depth
 * z_n passes bit 0's test and |z_n - z0| <= max_depth_jump, and with pc(n) = (dcx_n z_n, dcy_n z_n, z_n), a = pc(R) - pc(L),
 * b = pc(D) - pc(U), n = b x a (towards the camera, as the raycaster's normal on a surface seen from its front; not
 * normalised), l2 = |n|^2 is finite and > 0.
 * Flag bit 4 (16): bits 0 to 3 are set and the frame normal exists.  Bit 5 (32): bit 4 is set and, with nw = R n,
 * d = nw . nm, m2 = |nm|^2: d > 0 and d d >= ((min_normal_cos min_normal_cos) l2) m2.  With the gate on a pixel is valid
 * iff flags == 63; with it off nothing changes (flags <= 15, valid iff 15).  r, assoc, the Jacobian (still with the model
 * normal), the Huber weight, the sums and their order, the solve, levels, stops, statuses, results and log records are
 * untouched.  All f32, the order of operations fixed in tf_align_icp_gate.hip and restated in tests/align_icp_gate_ref.py.
 * The normal is formed in the rows launch, every evaluation: no normal map, no further launch.
 * The defaults are KinectFusion's 20 degrees and a round number; neither is tuned on recorded data.
 * Not here: a per-call form of the gate, a gate for tf_align_frame's SDF stage.  (A depth pyramid: the section below.) */
typedef struct tf_align_icp_gate {
  float min_normal_cos;   /* in [0, 1] */
  float max_depth_jump;   /* metres, > 0; +inf allowed: no discontinuity test */
} tf_align_icp_gate;
TF_API int tf_align_icp_gate_default(tf_align_icp_gate* out);          /* cosf(20 deg) = 0.9396926f, 0.1f */
/* gate == NULL: off.  TF_ERR_INVALID, with nothing changed, for a NaN, a cosine outside [0, 1], or a jump that is not > 0.
 * The setter and the getter launch nothing and wait for nothing; calls already enqueued keep the setting they were
 * enqueued with.  *on = 0 / 1; *out = the gate that is set, or the defaults where none is. */
TF_API int tf_align_icp_set_gate(tf_volume* v, const tf_align_icp_gate* gate);
TF_API int tf_align_icp_get_gate(tf_volume* v, tf_align_icp_gate* out, int32_t* on);
/* The frame's own normals, a pure function of the image, the camera, params->geo (stride[0], depth range) and *gate
 * (max_depth_jump; not the handle's setting): n f32 planar [3][H][W], camera frame, NOT normalised, 0 where there is none
 * or the pixel is not sampled.  It does not look at the model.  Read-only.  _device: asynchronous on the handle's stream;
 * the host form stages through the scratch pool and waits once.  TF_ERR_INVALID (nothing launched, nothing written) for a
 * null pointer, parameters tf_align_frame rejects (iters are not read) or a gate tf_align_icp_set_gate rejects. */
TF_API int tf_align_icp_frame_normals_device(tf_volume* v, const float* d_depth, const tf_align_icp_params* params,
                                             const tf_align_icp_gate* gate, float* d_normal3);
TF_API int tf_align_icp_frame_normals(tf_volume* v, const float* depth, const tf_align_icp_params* params,
                                      const tf_align_icp_gate* gate, float* normal3);

/* ---- the projective ICP on a depth pyramid (tf_align_icp_pyramid.hip) ---------------------------
 * Without it a level of stride s reads every s-th pixel of the full image against a model map of the full camera: the
 * coarse levels see the sensor's noise undiminished.  With it a level of stride s = 2^l is an image of its own, W >> l x
 * H >> l pixels, every pixel the mean of a 2 x 2 block of the level below, with a camera of its own and model maps raycast
 * for that camera: KinectFusion's form.  A setting of the handle, off in a new handle and off again after
 * tf_volume_reset.  The calls that run the projective ICP and raycast the model themselves read it: tf_align_frame_icp,
 * tf_align_icp_residuals where both maps are NULL, tf_track_frame, tf_track_frame_device, tf_track_integrate_device,
 * tf_track_texture_device, tf_relocalise.  The forms that take the caller's maps do not (those maps are of the full
 * camera): tf_align_frame_icp_device, tf_align_icp_residuals(_device) with maps.  tf_align_frame keeps its strides.
 * Level 0 is the caller's image.  Pixel (X, Y) of level l from a = (2X, 2Y), b = (2X + 1, 2Y), c = (2X, 2Y + 1),
 * d = (2X + 1, 2Y + 1) of level l - 1: valid iff all four are finite and > 0 and max - min of the four <= max_depth_jump
 * (one f32 subtraction); the value is ((a + b) + (c + d)) * 0.25f, every operation rounded on its own, else 0.  A mean
 * over whichever readings are valid would move the sample off the block's centre ray, so there is none.
 * The level camera, from the int-truncated intrinsics (fx, fy, cx, cy) of the image's camera and s = 2^l: fx / s, fy / s,
 * (cx + 1) / s - 1, (cy + 1) / s - 1 (the centre of the block 2X, 2X + 1 is 2X + 0.5, and pixel x has its centre at x with
 * the principal point at cx + 0.5); not truncated again.
 * A call with the setting on: every geo.stride[l], l < n_levels, must be 1, 2, 4 or 8 and divide W and H, otherwise
 * TF_ERR_INVALID, nothing launched, outputs untouched.  One launch builds every level image the schedule needs; one
 * raycast launch per distinct stride renders that level's maps (stride 1: the raycast of a call with the setting off);
 * then 1 + 2 launches per evaluation as ever, all enqueued up front, nothing read back.  A level evaluates every pixel of
 * its image against its maps with the rows kernel as it is (with tf_align_icp_set_gate on: the gated one, whose
 * neighbours are then the level image's adjacent pixels).  Flag bits, Huber weight, sums and their order, the solve,
 * stops, statuses, the closing evaluation, result and log are untouched; n_sampled is the level's pixel count and a
 * record's stride still names the level.  tf_align_icp_residuals writes level pixel (X, Y) at (sX, sY) of its full-size
 * maps, s = stride[0]; assoc = v * (W / s) + u in the level's model map; every other pixel gets 0, 0, -1.  With the
 * setting off every call is what it was, bit for bit.  tests/align_icp_pyramid_ref.py restates it.
 * The default jump is the gate's, a round number not tuned on recorded data.
 * Not here: a pyramid for tf_align_frame and tf_align_frame_color, for tf_align_group, for caller-supplied maps; image
 * sizes that 2^l does not divide; a blurred (Gaussian) pyramid; re-rendering the maps between levels. */
typedef struct tf_align_icp_pyramid {
  float max_depth_jump;   /* metres, > 0; +inf allowed: no spread test */
} tf_align_icp_pyramid;
TF_API int tf_align_icp_pyramid_default(tf_align_icp_pyramid* out);   /* 0.1f */
/* p == NULL: off.  TF_ERR_INVALID, with nothing changed, for a NaN or a jump that is not > 0.  The setter and the getter
 * launch nothing and wait for nothing; calls already enqueued keep the setting they were enqueued with.  *on = 0 / 1;
 * *out = the setting, or the defaults where there is none. */
TF_API int tf_align_icp_set_pyramid(tf_volume* v, const tf_align_icp_pyramid* p);
TF_API int tf_align_icp_get_pyramid(tf_volume* v, tf_align_icp_pyramid* out, int32_t* on);
/* cam4 = (fx, fy, cx, cy) and the size of level `level` (0..3) of the aligners' camera (tf_raycast_camera's where set, else
 * tf_set_camera's).  TF_ERR_INVALID for a null pointer, no camera, a level outside 0..3 or one the size does not allow. */
TF_API int tf_align_icp_pyramid_camera(tf_volume* v, int32_t level, float cam4[4], int32_t* width, int32_t* height);
/* Levels 1..n_levels (n_levels 1..3) of a depth image by *p (not the handle's setting): d_levels[l - 1] receives
 * f32[H >> l][W >> l]; entries past n_levels are not read.  One launch, read-only on the handle.  _device: asynchronous
 * on the handle's stream; the host form stages through the scratch pool and waits once.  TF_ERR_INVALID (nothing
 * launched, nothing written) for a null pointer, no camera, n_levels outside 1..3, a size 2^n_levels does not divide, or a
 * setting tf_align_icp_set_pyramid rejects. */
TF_API int tf_align_icp_pyramid_depth_device(tf_volume* v, const float* d_depth, int32_t n_levels,
                                             const tf_align_icp_pyramid* p, float* const d_levels[3]);
TF_API int tf_align_icp_pyramid_depth(tf_volume* v, const float* depth, int32_t n_levels, const tf_align_icp_pyramid* p,
                                      float* const levels[3]);

/* ---- the projective ICP held inside a plane: a photometric row from the model (tf_align_icp_color.hip) ----
 * On a wall, a floor or a table top the point-to-plane rows leave three degrees of freedom open: tf_align_frame_icp ends
 * TF_ALIGN_SINGULAR, or slides with its start where little relief is in view.  tf_align_frame_color cures that only inside
 * the truncation band.  These calls put a photometric row beside the ICP's: the model's intensity L at the vertex of each
 * model pixel (tf_align_frame_color's intensity, sampled from the volume, in [0, 1]; -1 on a miss or where a corner has no
 * colour), its central image differences Gu, Gv (only across neighbours that have an intensity and lie within
 * max_depth_jump in model depth), made once per call from the call's vertex and normal maps; per sampled pixel
 * rc = (L[i] + Gu[i] du + Gv[i] dv) - Lf at the associated model pixel i, (du, dv) the projection's offset from that
 * pixel's centre, Lf the frame pixel's luma; the gradient carried through the projection into the world frame and
 * tf_align_frame's twist.  Flag bits 0 to 3 (4, 5 with tf_align_icp_set_gate) are the plain call's; bit 8 (256): valid
 * geometrically, frame alpha != 0, model pixel usable; bit 9 (512): and |rc| <= max_photo_residual, the pixel is valid
 * photometrically.  Sums, the joined system M = A_g + w^2 A_c, the solve, stops, tf_align_color_result and
 * tf_align_color_iter are tf_align_frame_color's; TF_ALIGN_TOO_FEW goes by the geometric count.  With photo_weight == 0 or
 * on a volume without colour pose, status and every geometric sum are tf_align_frame_icp's, bit for bit, gate off or on.
 * All f32, the order of operations fixed in tf_align_icp_color.hip and restated in tests/align_icp_color_ref.py.  Readers:
 * no voxel, mark or model generation changes; state and log are their own, so tf_align_log, tf_align_color_log,
 * tf_align_icp_log and tf_align_group_log keep their meaning.
 * Not here: the depth pyramid (tf_align_icp_set_pyramid is not read by these calls; a level samples by stride), a
 * device-pose form (tf_track_*_device), a tf_relocalise hook, blurred images, multi-rank (exposure: tf_align_set_exposure). */
typedef struct tf_align_icp_color_params {
  tf_align_icp_params icp;
  float photo_weight, max_photo_residual, huber_photo; /* as tf_align_color_params'; all finite and >= 0 */
  float max_depth_jump;                                /* model depth across which no gradient is formed; > 0, +inf allowed */
} tf_align_icp_color_params;
typedef struct tf_track_color_result {
  tf_align_color_result icp, sdf;   /* sdf.geo.status == -1 (the rest 0): the second stage was not run */
  int32_t stage;                    /* 0 none usable, 1 colour icp only, 2 tf_align_frame_color */
  float pose[12];
} tf_track_color_result;
/* tf_align_icp_default_params, then 0.1, 0.25, 0.05 (tf_align_color_default_params') and max_depth_jump 0.1
 * (tf_align_icp_gate_default's).  None of these is tuned on recorded data. */
TF_API int tf_align_icp_color_default_params(tf_align_icp_color_params* out);
/* TF_ERR_INVALID (nothing launched, outputs untouched) for everything tf_align_frame_icp(_device) rejects, a null rgba (the
 * device form: not 4-byte aligned), non-finite or negative photo parameters, max_depth_jump not > 0.
 * _device: depth, RGBA8 [H][W][4], the caller's vertex and normal maps in device memory, model_pose on the host (not NULL);
 * asynchronous on the handle's stream, nothing read back.  tf_align_frame_icp_color: host images staged through the
 * scratch pool; the model is raycast at model_pose (NULL: at pose) into maps the handle owns; it waits once. */
TF_API int tf_align_frame_icp_color_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                           const float* d_model_vertex, const float* d_model_normal,
                                           const float model_pose[12], const tf_align_icp_color_params* params,
                                           tf_align_color_result* d_result);
TF_API int tf_align_frame_icp_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                    const float* model_pose, const tf_align_icp_color_params* params,
                                    tf_align_color_result* result);
/* the records of the last tf_align_frame_icp_color(_device) or tf_track_frame_color call (waits for it), as tf_align_color_log */
TF_API int tf_align_icp_color_log(tf_volume* v, tf_align_color_iter* out, int64_t cap, int64_t* n);
/* The maps of one evaluation at icp.geo.stride[0] (iters are not read): r, flags, assoc as tf_align_icp_residuals', rc
 * f32[H][W] and the world-frame gradient gradc3 f32[3][H][W] (both 0 without bit 8); any may be NULL; pixels not sampled
 * get 0, 0, 0, -1, 0.  The host form takes host maps, or raycasts the model where both are NULL. */
TF_API int tf_align_icp_color_residuals(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                        const float* model_vertex, const float* model_normal, const float* model_pose,
                                        const tf_align_icp_color_params* params, float* r, float* rc, uint32_t* flags,
                                        int32_t* assoc, float* gradc3);
TF_API int tf_align_icp_color_residuals_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                               const float* d_model_vertex, const float* d_model_normal,
                                               const float model_pose[12], const tf_align_icp_color_params* params,
                                               float* d_r, float* d_rc, uint32_t* d_flags, int32_t* d_assoc, float* d_gradc3);
/* A diagnostic, as tf_align_icp_frame_normals is: the model maps a call would make of these vertex and normal maps --
 * L, Gu, Gv, each f32[H][W], any may be NULL; a gradient that does not exist is a quiet NaN.  TF_ERR_INVALID for a null
 * input, a non-finite model pose, parameters the calls above reject (iters are not read). */
TF_API int tf_align_icp_color_model_maps(tf_volume* v, const float* model_vertex, const float* model_normal,
                                         const float model_pose[12], const tf_align_icp_color_params* params, float* L,
                                         float* Gu, float* Gv);
TF_API int tf_align_icp_color_model_maps_device(tf_volume* v, const float* d_model_vertex, const float* d_model_normal,
                                                const float model_pose[12], const tf_align_icp_color_params* params,
                                                float* d_L, float* d_Gu, float* d_Gv);
/* tf_track_frame with colour in both stages: tf_align_frame_icp_color with the model raycast at the start pose; where that
 * ends with status <= TF_ALIGN_MAX_ITERS, tf_align_frame_color from its pose; out->stage and out->pose by tf_track_frame's
 * rule.  It waits twice.  TF_ERR_INVALID (nothing launched, out untouched) for what either stage rejects. */
TF_API int tf_track_frame_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                const tf_align_icp_color_params* icp_params, const tf_align_color_params* sdf_params,
                                tf_track_color_result* out);

/* ---- exposure compensation in the photometric aligners (tf_align_exposure.hip) -------------------
 * A camera with auto-exposure shows the model brighter or darker than the volume's running mean holds it.  With this
 * setting the frame's luma is compensated before it is compared, in f32, every operation rounded on its own:
 *   Lfe = gain_f * Lf + offset_f;   rc = L(pw) - Lfe  (tf_align_frame_color),
 *   rc = (L[i] + (Gu[i] du + Gv[i] dv)) - Lfe  (tf_align_frame_icp_color)
 * with Lf formed as before and (gain_f, offset_f) the f32 roundings of a pair carried in f64 beside the pose.  Every flag
 * bit keeps its definition; bit 6 (bit 9 of the ICP form) and the Huber weight use the compensated rc.  With gain 1 and
 * offset 0, Lfe is Lf bit for bit.  The pair is estimated with the pose: a third row of 17 sums beside the geometric and
 * the photometric one (P_i = sum wJc_i, Q_i = sum wJc_i Lf, S_w = sum wc, S_l = sum wc Lf, S_ll = sum wl Lf, S_r = sum wc rc,
 * S_lr = sum wl rc with wl = wc * Lf, each term the f64 product of two f32 operands, over the photometrically valid
 * pixels), the pair eliminated from the photometric system ahead of the joined 6 x 6 solve and stepped after it
 * (tf_align_exposure_solve.h states every operation; tests/align_exposure_ref.py restates it).  Stops, TF_ALIGN_TOO_FEW by
 * the geometric count, the convergence test on the twist alone and the closing evaluation are unchanged; with
 * photo_weight == 0 or on a volume without colour pose, status and geometric sums stay the plain call's bit for bit.
 * A setting of the handle, as tf_align_icp_set_gate: off in a new state and off again after tf_volume_reset.  It is read by
 * tf_align_frame_color(_device), tf_align_frame_icp_color(_device), both residual-map calls (their rc uses the cell's
 * current pair) and tf_track_frame_color.  The start pair lives in a cell in device memory the handle owns: the setter
 * writes (gain0, offset0) into it on the handle's stream, a call's begin launch reads its start from it, and with carry on
 * the closing solve launch of a call that ends with status <= TF_ALIGN_MAX_ITERS writes its estimate there (a call stopped
 * TF_ALIGN_TOO_FEW or TF_ALIGN_SINGULAR leaves the cell as it was): the _device forms stay asynchronous, nothing is read
 * back.  tf_track_frame_color's second stage starts from its first stage's estimate whenever it runs, whatever carry says;
 * after the call the cell holds the last stage's estimate with carry on and (gain0, offset0) with carry off.  With the
 * setting off every call enqueues exactly the launches it enqueued before.
 * Not here: per-channel gains, vignetting, response curves, the group aligner, use of the estimate by the integrator. */
typedef struct tf_align_exposure {
  int32_t unknowns;         /* 0: apply the start pair, estimate nothing; 1: the offset; 2: gain and offset */
  int32_t carry;            /* != 0: a call that ends with status <= TF_ALIGN_MAX_ITERS leaves its estimate as the next call's start */
  float gain0, offset0;     /* the start pair */
  float min_gain, max_gain; /* the gain is clamped into this after every update */
} tf_align_exposure;
typedef struct tf_align_exposure_iter {   /* one per evaluation, parallel to the tf_align_color_iter of the same index */
  double gain, offset;                    /* the pair at which the sums were taken */
  int32_t rank, n_photo;                  /* unknowns eliminated in this evaluation (0..2); photometrically valid pixels */
  double P[6], Q[6], S_w, S_l, S_ll, S_r, S_lr;
  double d_offset, d_gain;                /* the step taken on the pair, 0 where none was taken */
} tf_align_exposure_iter;
/* unknowns 2, carry 0, gain0 1, offset0 0, min_gain 0.25, max_gain 4.  None of these is tuned on recorded data. */
TF_API int tf_align_exposure_default(tf_align_exposure* out);
/* e == NULL: off.  TF_ERR_INVALID (setting unchanged, nothing launched) for unknowns outside 0..2, a non-finite field,
 * min_gain <= 0, min_gain > max_gain, gain0 outside [min_gain, max_gain]. */
TF_API int tf_align_set_exposure(tf_volume* v, const tf_align_exposure* e);
TF_API int tf_align_get_exposure(tf_volume* v, tf_align_exposure* out, int32_t* on);
/* which: 0 the last tf_align_frame_color(_device) call, 1 the last tf_align_frame_icp_color(_device) or
 * tf_track_frame_color call; TF_ERR_INVALID outside 0..1.  Both wait for the call, as the other logs.  The log holds the
 * records of that call where it ran with the setting on (*n = 0 otherwise).  The estimate is the pair that call ended at,
 * *valid != 0 where it ran with the setting on and ended with status <= TF_ALIGN_MAX_ITERS. */
TF_API int tf_align_exposure_log(tf_volume* v, int32_t which, tf_align_exposure_iter* out, int64_t cap, int64_t* n);
TF_API int tf_align_exposure_estimate(tf_volume* v, int32_t which, double gain_offset[2], int32_t* valid);

/* ---- tracking and integrating with the pose kept on the device (tf_devpose.hip) ------------------
 * KinectFusion's loop on the stream: track frame f against the model, decide whether the result is good enough, integrate
 * the frame at the tracked pose, track frame f + 1 from it -- everything enqueued up front, nothing read back; the host
 * looks at the results when it wants to.  The pose travels in a cell in device memory.  The device checks a cell, not the
 * host: a cell with valid == 0 or a non-finite entry holds no pose, every launch that depends on it does nothing, and the
 * outputs say so (below).  Cells are 16-byte aligned.
 * The textured unit runs from a cell too (tf_integrate_frame_textured_posed_device, tf_track_texture_device): the matrix the
 * patch stage projects with is the cell's rigid inverse, taken on the device.  Not here: that patch stage as a part of the
 * next frame's launch (it is a launch of its own), a textured form for a handle with untextured marks pending, a multi-rank
 * form (a handle with a partition or a communicator is refused), a group or colour form of the device tracker, caching the
 * tracked frame as a keyframe. */
typedef struct tf_device_pose {   /* 64 bytes, 16-byte aligned, device memory */
  float   pose[12];               /* camera-to-world, row-major 3 x 4, as everywhere else */
  int32_t valid;                  /* 0: every launch that reads this cell returns at once */
  int32_t reserved[3];
} tf_device_pose;
typedef struct tf_track_accept {      /* tf_relocalise's test of a try */
  int32_t min_stage;                  /* 1 or 2 */
  float   min_valid_fraction;         /* of n_valid_last / n_sampled of the stage that gave the pose, in [0, 1] */
  float   max_rms;                    /* of that stage's rms_last, finite and >= 0 */
} tf_track_accept;
TF_API int tf_track_accept_default(tf_track_accept* out);   /* 2, 0.5, 0.01: tf_relocalise's defaults */
/* tf_track_frame with everything in device memory and no wait: the model raycast at *d_start, the ICP from it, the SDF
 * stage from the ICP's f32 pose where the ICP held (0 <= status <= TF_ALIGN_MAX_ITERS), *d_out as tf_track_frame fills
 * it, bit for bit.  The result is accepted where stage >= min_stage, and of the stage that gave the pose n_sampled > 0,
 * (float)n_valid_last >= min_valid_fraction * (float)n_sampled and rms_last <= max_rms -- tf_relocalise's expressions, by
 * the same function; accept == NULL: where stage >= 1.  *d_pose_out = {d_out->pose, valid 1} where it is accepted, else
 * {the start cell's 12 floats, valid 0}.  d_pose_out may be d_start.
 * A start cell that holds no pose: *d_out = {icp.status -1, sdf.status -1, the rest of both 0, stage 0, pose = the cell's
 * 12 floats as stored}, d_pose_out->valid = 0.  A stage that did not run has no records of this call: tf_align_icp_log
 * then returns none, tf_align_log (as after tf_track_frame) those of the last call that ran it; otherwise both return
 * this call's records.
 * TF_ERR_INVALID (nothing launched, outputs untouched) for what tf_track_frame rejects from its parameters, a null
 * pointer, a cell that is not 16-byte aligned, accept fields out of range, a raycast camera whose size is not
 * tf_set_camera's (tf_relocalise's rule), a handle with a partition or a communicator.  Only the pose checks are made on
 * the device. */
TF_API int tf_track_frame_device(tf_volume* v, const float* d_depth, const tf_device_pose* d_start,
                                 const tf_align_icp_params* icp, const tf_align_params* sdf,
                                 const tf_track_accept* accept, tf_track_result* d_out, tf_device_pose* d_pose_out);
/* tf_integrate_frames_device for one frame whose pose is *d_pose; d_rgba may be NULL.  The volume afterwards is that
 * call's with the same pose, and so is the handle: epoch, selection-set rotation, dirty marks, the bound frame; selections
 * made ahead by a streaming call are discarded, as for a stream that changed course.  A cell that holds no pose: the
 * volume is untouched, and the frame counts as one that selected nothing (tf_get_stats: n_selected, n_coarse and the id
 * range are 0).  TF_ERR_INVALID for a null depth or cell pointer, misaligned images or cell, a partition or a communicator. */
TF_API int tf_integrate_frame_posed_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                           const tf_device_pose* d_pose);
/* the two above in sequence on the handle's stream, the frame integrated at *d_pose_out only where it was accepted */
TF_API int tf_track_integrate_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                     const tf_device_pose* d_start, const tf_align_icp_params* icp,
                                     const tf_align_params* sdf, const tf_track_accept* accept,
                                     tf_track_result* d_out, tf_device_pose* d_pose_out);
/* diagnostic: the constants block the selection launches read, derived from *d_pose as the device wrote it (waits once).
 * Words of 4 bytes, in order: res, id_factor, step (i32), diag, diag_step, dtn_coarse, dtn_fine, rot[3][3], tc[3], r0[3],
 * r1[3], r2[3], coarse[3][8], fine[3][8], pose[12], resDiag, plain (i32) -- tf_host_math.h's SelectConsts -- then the
 * pose again (12), the gate word (i32, 1: the cell held a pose) and 3 words of padding: 424 bytes; the first `bytes`
 * (<= 424) are copied. */
TF_API int tf_pose_consts_download(tf_volume* v, const tf_device_pose* d_pose, void* out, size_t bytes);
/* The textured unit for one frame whose pose is *d_pose.  With pose = the cell's 12 floats and T its rigid inverse
 * [R^T | -R^T t; 0 0 0 1] -- row-major, T[4r + c] = pose[4c + r], T[4r + 3] = (float)-((p[r] p[3] + p[4 + r] p[7]) +
 * p[8 + r] p[11]) with the products and the two additions in double -- the volume, meshes, patches, atlas and handle
 * afterwards are those of tf_stream_frames_textured_device(v, 1, 0, &d_depth, &d_rgba, pose, T, frame_id), bit for bit; the
 * frame's patch stage is on the stream when the call returns.  Selections made ahead by a streaming call are discarded; a
 * patch stage such a call left pending is carried as by any frame.  A cell that holds no pose: volume, dirty set, meshes,
 * patches, atlas texels and the atlas's next location are untouched, tf_get_stats' last-frame figures are 0 as after
 * tf_integrate_frame_posed_device, and the handle's host-side counters advance.
 * TF_ERR_INVALID (nothing of this frame launched, outputs untouched, tf_last_error says which) for what
 * tf_integrate_frame_posed_device refuses, a null d_rgba, a texture stage half done (tf_texture_frame_device_phase), and a
 * handle on which frames integrated without texturing still wait for a mesher: the host cannot know whether the cell holds
 * a pose, and if it does not, the backlog would be meshed and its marks cleared without patches.  Texture the backlog
 * first (tf_texture_frame_device). */
TF_API int tf_integrate_frame_textured_posed_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                                    const tf_device_pose* d_pose, int32_t frame_id);
/* tf_track_frame_device, then the call above at *d_pose_out: the frame is integrated and textured only where it was
 * accepted.  Everything either call refuses is refused before anything is launched. */
TF_API int tf_track_texture_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba,
                                   const tf_device_pose* d_start, const tf_align_icp_params* icp,
                                   const tf_align_params* sdf, const tf_track_accept* accept,
                                   tf_track_result* d_out, tf_device_pose* d_pose_out, int32_t frame_id);
/* diagnostic: the block the posed patch stage reads, derived from *d_pose as the device wrote it (waits once): T[16] as
 * above (f32), the gate word (i32, 1: the cell held a pose) and 3 words of padding: 80 bytes; the first `bytes` (<= 80)
 * are copied.  With the gate off T is the same arithmetic on whatever the cell stores. */
TF_API int tf_pose_inverse_download(tf_volume* v, const tf_device_pose* d_pose, void* out, size_t bytes);

/* ---- relocalising a lost camera against the cached keyframes (tf_reloc.hip) -------------------
 * tf_track_frame needs a start within the ICP's capture range (about 12 cm / 8 degrees).  A caller that has none asks the
 * keyframes the handle already holds (tf_keyframe_cache(_device), tf_keyframe_set_pose): which of them look like this
 * frame (retrieval over small images, on the device), and does the tracker hold from one of their poses (verification,
 * tf_track_frame as it is).
 * Descriptor of an image of the integrator's camera (tf_set_camera, W x H): tiny_w x tiny_h blocks of bw x bh =
 * (W / tiny_w) x (H / tiny_h) pixels, n = tiny_w * tiny_h, block i = by * tiny_w + bx.  All integers:
 *   G[i] = sum over the block of 77 R + 150 G + 29 B (u32);  S = sum of G (u64)
 *   a pixel counts where its depth z is finite and min_depth <= z <= max_depth; mm = (u32)rintf(z * 1000.0f), both f32;
 *   c = pixels that count;  Z[i] = (sum of mm) / c (integer division) where 2 c >= bw bh, else -1 (i32)
 * Score of a query q against a row k (texturefusion_amd/csrc/tf_reloc_score.h holds the f64 expressions):
 *   D_i = G_i(q) - G_i(k);  N = n sum D_i^2 - (sum D_i)^2, an exact integer;  s_grey = N / (n^2 (256 bw bh)^2): the
 *   zero-mean SSD in grey levels squared, unchanged exactly by a uniform brightness offset that saturates nowhere
 *   m = blocks with Z >= 0 in both;  s_depth = sum over them of (Z_i(q) - Z_i(k))^2 / m * 1e-6 (metres squared)
 *   score = grey_weight s_grey + depth_weight s_depth;  m < min_overlap: +inf, not a candidate
 * Candidates are ranked by ascending score, then ascending kf_id.  The index lives in the handle.  A row is the image as it
 * was when added: a caller who caches a keyframe again, or changes images it owns, adds it again.  A row whose keyframe
 * has been released since, or has no pose (tf_keyframe_set_pose), is skipped by a query.  tf_volume_reset frees the index
 * and its configuration.  Read-only on the volume, the atlas and the keyframe table.
 * Not here: invariance to a rotation about the optical axis, features of any kind, a multi-rank form. */
typedef struct tf_reloc_params {
  int32_t tiny_w, tiny_h;          /* blocks across and down; W % tiny_w == 0 and H % tiny_h == 0 */
  float min_depth, max_depth;      /* max_depth <= 60 */
  float grey_weight, depth_weight; /* >= 0 */
  int32_t min_overlap;             /* >= 0 */
} tf_reloc_params;
/* 40 x 30 blocks, depth in [0.05, 5], weights 1 and 2.55e4, min_overlap 300 (n / 4) */
TF_API int tf_reloc_default_params(tf_reloc_params* out);
/* Sets the descriptor and the score, and empties the index.  TF_ERR_INVALID where the grid does not divide the camera, a
 * block holds more than 65536 pixels, a parameter is out of range or there is no camera.  The configuration belongs to the
 * camera it was made for: after a tf_set_camera to another size every call below is refused until it is made again. */
TF_API int tf_reloc_configure(tf_volume* v, const tf_reloc_params* params);
/* Describes the named cached keyframes in one launch and puts them into the index; a keyframe that is there already gets
 * its row replaced.  An id that is not cached: TF_ERR_INVALID, nothing changes.  Asynchronous. */
TF_API int tf_reloc_index_add(tf_volume* v, const int32_t* kf_ids, int64_t n);
/* ids that are not in the index are passed over */
TF_API int tf_reloc_index_remove(tf_volume* v, const int32_t* kf_ids, int64_t n);
TF_API int tf_reloc_index_clear(tf_volume* v);
TF_API int tf_reloc_index_count(tf_volume* v, int64_t* n);
/* The descriptor of host images (depth f32[H][W], rgb u8[H][W][rgb_pixel_stride], stride 3 or 4) -> G u32[n], Z i32[n], *S;
 * and the row of an indexed keyframe (TF_ERR_INVALID where it is not in the index).  Both wait once. */
TF_API int tf_reloc_describe(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride, uint32_t* G,
                             int32_t* Z, uint64_t* S);
TF_API int tf_reloc_descriptor_download(tf_volume* v, int32_t kf_id, uint32_t* G, int32_t* Z, uint64_t* S);
/* The candidates for a frame, ranked: *n = how many there are, the first min(*n, cap) written (any output may be NULL).
 * One describe launch, one score launch over every row, one download of 12 bytes per row, one wait; the host ranks. */
TF_API int tf_reloc_query(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride,
                          int32_t* out_kf_ids, double* out_scores, int32_t* out_overlap, int64_t cap, int64_t* n);
TF_API int tf_reloc_query_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgb, int32_t rgb_pixel_stride,
                                 int32_t* out_kf_ids, double* out_scores, int32_t* out_overlap, int64_t cap, int64_t* n);

#define TF_RELOC_FOUND 0
#define TF_RELOC_NOT_FOUND 1     /* candidates, but no try passed */
#define TF_RELOC_NO_CANDIDATE 2  /* an empty index, or no row with a finite score */
#define TF_RELOC_MAX_TRIES 8
typedef struct tf_relocalise_params {
  int32_t max_tries;          /* 1 .. TF_RELOC_MAX_TRIES */
  int32_t min_stage;          /* 1 or 2: the tf_track_result.stage a try has to reach */
  float min_valid_fraction;   /* of n_valid_last / n_sampled of the stage that gave the pose, in [0, 1] */
  float max_rms;              /* of that stage's rms_last, metres */
  tf_align_icp_params icp;    /* tf_track_frame's */
  tf_align_params sdf;
} tf_relocalise_params;
typedef struct tf_reloc_try {
  int32_t kf_id, overlap;
  double score;
  tf_track_result track;
} tf_reloc_try;
typedef struct tf_relocalise_result {
  int32_t status;    /* TF_RELOC_* */
  int32_t kf_id;     /* FOUND: the keyframe the accepted try started from; NOT_FOUND: the best-ranked one; else -1 */
  int32_t rank;      /* FOUND: that keyframe's rank among the candidates (0 = best); else -1 */
  int32_t n_tried;
  float pose[12];    /* FOUND: the tracker's pose; NOT_FOUND: the best-ranked keyframe's pose; else 0 */
  tf_reloc_try tries[TF_RELOC_MAX_TRIES];
} tf_relocalise_result;
/* max_tries 3, min_stage 2, min_valid_fraction 0.5, max_rms 0.01, the stages' own defaults */
TF_API int tf_relocalise_default_params(tf_relocalise_params* out);
/* tf_reloc_query, then tf_track_frame(depth, pose_k, icp, sdf) for the candidates in rank order, at most max_tries of them,
 * until one is accepted: stage >= min_stage, and of the stage that gave its pose n_valid_last >= min_valid_fraction *
 * n_sampled and rms_last <= max_rms.  pose_k is the rigid inverse of the keyframe's pose_inv16, [R^T | -R^T t], computed
 * in f64 and rounded to f32.  The status is a field of the result: a call that finds nothing returns TF_OK.  It waits
 * once for the query and twice per try.  TF_ERR_INVALID (nothing launched, the result untouched) for what either tracker
 * stage rejects, a parameter out of range, no configured index, or a raycast camera (tf_raycast_camera) whose size is not
 * tf_set_camera's: the tracker would read the frame at that size. */
TF_API int tf_relocalise(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride,
                         const tf_relocalise_params* params, tf_relocalise_result* result);

/* ---- meshing (the stage between the volume and the atlas) -----
 * Chisel::UpdateMeshes (Structure/Chisel.h:479-481) -> ChunkManager::RecomputeMeshes
 *   (Structure/ChunkManager.cpp:232-264): every chunk of meshesToUpdate that exists is re-meshed by
 *   GenerateMeshEfficient (:595-1002, gradient normals :277-455) on the device; meshes stay in HBM
 *   (ChunkManager::allMeshes).  *n_meshed = size of the dirty set handed to the mesher. */
TF_API int tf_update_meshes(tf_volume* v, int64_t* n_meshed);
/* Diagnostic of the filter ahead of the mesher.  The library keeps per chunk a 16-bit summary of the classes
 *   (observed / positive / negative / weight > 50, i.e. what GenerateMeshEfficient's per-cell tests at
 *   ChunkManager.cpp:669-722 and :776-777 ask for) that occur among its voxels and on its three low faces; a chunk
 *   whose summaries rule out a vertex is not read at all.  A summary must be a superset of the truth: *n_missing =
 *   chunks whose voxels hold a class the summary lacks (must be 0), *n_stale = chunks whose summary holds a class the
 *   voxels no longer do (allowed: costs time, never changes a result).  Any output may be NULL. */
TF_API int tf_check_summaries(tf_volume* v, int64_t* n_chunks, int64_t* n_missing, int64_t* n_stale);
/* Diagnostic of the neighbour table the filter and the patch stage read instead of probing the chunk hash (what
 *   ChunkManager::GenerateMeshEfficient resolves per call with GetChunk on the neighbour ids, Structure/ChunkManager.cpp:618-632,
 *   and Chisel::CompressMeshes with allMeshes.find, Structure/Chisel.cpp:134-137): per pool slot the pool slots of the 26
 *   chunks around it, filled lazily.  out6 = {rows, non-zero words, non-zero words that disagree with the hash (must be 0),
 *   rows whose "no chunk there" words are currently trusted, trusted "none" words whose chunk exists (must be 0), 0}. */
TF_API int tf_check_neighbours(tf_volume* v, int64_t out6[6]);
/* keys of ChunkManager::GetAllMeshes() (Structure/ChunkManager.h:714) */
TF_API int tf_list_meshes(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n);
/* Mesh::vertices.size() / indices.size() / adj[6] / simplified of listed chunks (Mesh.h:70-85);
 *   TF_ERR_MISSING_CHUNK when a chunk has no mesh (allMeshes.at() throws).  Outputs may be NULL. */
TF_API int tf_mesh_counts(tf_volume* v, const int32_t* ids, int64_t n, int32_t* n_vertices,
                          int32_t* n_indices, uint8_t* adj, uint8_t* simplified);
/* Mesh::vertices / normals / colors (Vec3List: 3 f32 per vertex) and Mesh::indices of listed chunks,
 *   packed by the caller's running offsets (vert_offsets[n+1], index_offsets[n+1] from tf_mesh_counts). */
TF_API int tf_meshes_download(tf_volume* v, const int32_t* ids, int64_t n, const int64_t* vert_offsets,
                              const int64_t* index_offsets, float* verts, float* normals, float* colors,
                              uint32_t* indices);
/* Chisel::CompressMeshes(meshesToUpdate) (Structure/Chisel.cpp:112-147): Mesh::SimplifyByClustering's
 *   adjacency flags (geometry/Mesh.cpp:39-83) exchanged with the face neighbours, meshesToUpdate
 *   cleared.  out_ids receives tsdfFusion's chunksToUpdate -- the dirty keys that have a mesh
 *   (GCFusion/MobileFusion.cpp:345-353) -- in ascending (x, y, z) order (the reference's order is its
 *   unordered_map's iteration order, i.e. unspecified). */
TF_API int tf_compress_meshes(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n);

/* ---- measurement ------------------------------------------------------------------- */
/* kind_mask: bit k set = bracket every launch of kernel kind TF_PROF_k with a pair of HIP events
 * on the handle's stream (0 = off).  Timing only the dominant kernel keeps the event overhead
 * out of the other launches. */
TF_API int tf_profile_enable(tf_volume* v, uint32_t kind_mask);
TF_API int tf_profile_get(tf_volume* v, tf_profile* out, int reset);
/* What a HIP-event pair around an EMPTY launch reads on the handle's stream (microseconds, mean of n_pairs): the
 *   floor contained in every per-kernel time of tf_profile_get (launch + marker latency, not kernel work). */
TF_API int tf_profile_calibrate(tf_volume* v, int32_t n_pairs, double* us_per_pair);
/* Tuning aid: the raw per-wave timeline table (16 words per wave; words 10..13 = {start, end, role+1,
 * XCC id}, 14..15 = K-A prologue end / first list record loaded, in 100 MHz ticks) of the last
 * fused launch that ran all three roles; filled only while the environment variable TF_KA_DBG has
 * bit 12 (4096) set. */
TF_API int tf_debug_phase_raw(tf_volume* v, uint64_t* out, int64_t cap_words);

/* ---- multi-GPU chunk-range partition --------------------------------
 * A rank owns chunks with lo <= id.x < hi; selection runs in full on every rank, integrate /
 * finalize touch only owned chunks.  The chunks of the slab's ghost band that were updated since
 * the previous tf_boundary_pack are packed into / unpacked from a device buffer that is
 * all-gathered over RCCL.  Ghost band = what another rank's mesher reads of this slab: the layer
 * key == hi-1, and the layers lo <= key <= lo + (a+b+c) -- GenerateMeshEfficient reads c + {0,1}^3
 * (Structure/ChunkManager.cpp:618-632) and extractGradientFromCubic the face neighbours of those
 * (:288-315).  Record = 16 B header {x,y,z,update epoch} + 4 KiB {sdf,weight}[512] + 4 KiB colour[512][4].
 * A record that does not fit the buffer stays flagged (TF_ERR_CAPACITY; call again with more room). */
#define TF_BOUNDARY_RECORD_BYTES (16 + 4096 + 4096)
TF_API int tf_set_partition(tf_volume* v, int32_t x_lo, int32_t x_hi);
/* The same with the ownership key a*x + b*y + c*z (a, b, c in {0, 1}) instead of x: a rank owns
 * key_lo <= key < key_hi.  (1, 1, 1) cuts axis-aligned walls and floors diagonally, so no single
 * rank holds a whole wall (its ghost band is four layers thick on the lower side). */
TF_API int tf_set_partition_key(tf_volume* v, int32_t a, int32_t b, int32_t c, int32_t key_lo, int32_t key_hi);
TF_API int tf_boundary_pack(tf_volume* v, void* d_records, int64_t cap_records, int64_t* n);
/* The same without a host round trip: the record count (which may exceed cap_records; only the first
 * cap_records were written) lands in the device word *d_count, ordered on the handle's stream, so
 * that the exchange of one frame batch can overlap the integration of the next. */
TF_API int tf_boundary_pack_async(tf_volume* v, void* d_records, int64_t cap_records, uint32_t* d_count);
TF_API int tf_boundary_unpack(tf_volume* v, const void* d_records, int64_t n_records);
/* Fixed-capacity form for a single collective without a host round trip: a block is
 *   [u32 record count, 12 B padding | cap_records records]   (tf_boundary_block_bytes(cap) bytes);
 * tf_boundary_pack_block fills this rank's block (the count may exceed cap_records: the surplus stays flagged
 * for the next exchange and the receivers report TF_ERR_CAPACITY at their next synchronising call);
 * tf_boundary_unpack_blocks consumes the all-gathered blocks of every rank but own_block; join_dirty != 0
 * (between the voxel update of a frame and tf_texture_frame_device): the owned face neighbours of every ghost
 * that arrives join that frame's dirty set -- their neighbour was updated on another rank.  Asynchronous. */
TF_API size_t tf_boundary_block_bytes(int64_t cap_records);
TF_API int tf_boundary_pack_block(tf_volume* v, void* d_block, int64_t cap_records);
TF_API int tf_boundary_unpack_blocks(tf_volume* v, const void* d_blocks, int32_t n_blocks, int32_t own_block,
                                     int64_t cap_records, int join_dirty);
/* Two blocks instead of one, for a neighbour-only exchange: slabs are contiguous key ranges, so the chunks the rank
 * BELOW reads as ghosts are those with key - key_lo <= a + b + c (d_block_down) and the rank ABOVE reads key == key_hi - 1
 * (d_block_up); a chunk of a thin slab goes to both.  Valid as the only exchange when every slab is at least
 * a + b + c + 1 keys wide.  Consume a neighbour's block with tf_boundary_unpack_blocks(..., own_block = -1, ...). */
TF_API int tf_boundary_pack_bands(tf_volume* v, void* d_block_down, void* d_block_up, int64_t cap_records);
/* The SIZED form of the neighbour exchange: blocks as large as what the frame can have changed, not a fixed capacity.
 * Every rank runs the same selection, so each one counts -- identically -- the selected chunks of its own two bands and of
 * the two neighbouring bands it receives (the selection role does it on the device for the frame integrated last by a
 * streaming entry point).  tf_boundary_band_bounds returns the four record capacities
 *     bounds = { send_down, send_up, recv_from_below, recv_from_above }
 * (counts rounded up to multiples of 8, at least 8, at most cap_records): rank r's send_down equals rank r - 1's
 * recv_from_above by construction, so both sides of a transfer post tf_boundary_block_bytes(bound) bytes without talking
 * to each other.  Selected chunks are a superset of updated ones, so nothing a frame flagged is left behind; whatever an
 * EARLIER overflow left flagged rides in the slack or waits (it stays flagged).  tf_boundary_band_bounds waits for the
 * device to publish the counts (it does not drain the stream).  tf_boundary_pack_bands2 / tf_boundary_unpack_pair are
 * pack_bands / unpack_blocks with one capacity per block and separately placed blocks.
 * Replaces nothing in the reference (single process); SURVEY.md s.8e. */
TF_API int tf_boundary_band_bounds(tf_volume* v, int64_t cap_records, int64_t bounds[4]);
TF_API int tf_boundary_pack_bands2(tf_volume* v, void* d_block_down, int64_t cap_down, void* d_block_up, int64_t cap_up);
TF_API int tf_boundary_unpack_pair(tf_volume* v, const void* d_from_below, int64_t cap_below, const void* d_from_above,
                                   int64_t cap_above, int join_dirty);
/* RCCL inside the library: one process per GPU.  tf_comm_unique_id on one rank, the 128 bytes
 * distributed by the host's own means, tf_comm_init(rank, nranks, id) on every rank (ncclCommInitRank);
 * tf_exchange_boundary = tf_boundary_pack_block -> ONE ncclAllGather over xGMI on the handle's stream ->
 * tf_boundary_unpack_blocks, nothing copied to the host.  tf_comm_exchange_every_frame(cap): the textured
 * per-frame flow (tf_stream_frames_textured_device / tf_integrate_frame_host) then exchanges after every
 * voxel update, ahead of the mesher; owned face neighbours of arriving ghost chunks join the frame's dirty set. */
TF_API int tf_comm_unique_id(void* out128);
TF_API int tf_comm_init(tf_volume* v, int rank, int nranks, const void* unique_id128);
TF_API int tf_comm_destroy(tf_volume* v);
TF_API int tf_exchange_boundary(tf_volume* v, int64_t cap_records);
TF_API int tf_comm_exchange_every_frame(tf_volume* v, int64_t cap_records);
/* How tf_exchange_boundary / the per-frame exchange move the blocks: TF_XCHG_NEIGHBOURS (default) = one grouped
 * ncclSend / ncclRecv pair with the rank below and the rank above (tf_boundary_pack_bands: a rank receives two blocks
 * whatever the number of ranks); TF_XCHG_ALLGATHER = one ncclAllGather of every rank's block.  The neighbour form
 * REQUIRES rank r's slab to sit directly above rank r - 1's (key_lo of r == key_hi of r - 1, the same key coefficients on
 * every rank) and every slab above the lowest to be at least a + b + c + 1 keys wide; the library checks this with one
 * 32-byte all-gather at the first exchange after tf_comm_init / tf_set_partition_key (a collective: every rank gets
 * there) and uses the all-gather form on ALL ranks when it does not hold.  The per-frame exchange of the neighbour form
 * is sized by the frame's selection (tf_boundary_band_bounds above); cap_records is then only the upper limit.
 * tf_comm_stats: exchanges run and bytes received by this rank so far.  tf_comm_stats_ex (synchronises): out =
 * { exchanges, bytes sent, bytes received, ghost records written into blocks, ghost records read from received blocks,
 *   record capacity of the blocks sent, the form in use (TF_XCHG_*), bit 0: the partition check has run | (exchanges that
 *   ran on the library's second stream next to an interior mesh pass) << 1 }. */
#define TF_XCHG_NEIGHBOURS 0
#define TF_XCHG_ALLGATHER 1
TF_API int tf_comm_exchange_mode(tf_volume* v, int mode);
TF_API int tf_comm_stats(tf_volume* v, int64_t* exchanges, int64_t* bytes_received);
TF_API int tf_comm_stats_ex(tf_volume* v, int64_t out[8]);

/* ---- texture atlas on device-resident meshes --------------------------------------------
 * Atlas / Patch (Structure/Atlas.{h,cpp}, Structure/Patch.{h,cpp}) as driven by Chisel::GeneratePatches /
 * CompensateColor / UpdateAtlas / DrawMeshes (Structure/Chisel.cpp:149-355).  Meshes (ChunkManager::allMeshes)
 * and their patches (Mesh::m_patch: texloc, frameid, boundingbox, ratio, texcoord, texcolor, labs) stay in
 * HBM; the host sees them through the *_download mirrors.
 *
 * tf_keyframe_cache: the reference keeps Frame::rgb / refined_depth alive and Patch::SetImage holds a
 *   non-owning ROI into it (Patch.cpp:172-175); here the keyframe's images are cached in HBM under kf_id
 *   (= the frame id view selection hands out as label).  rgb = u8[H][W][3], depth = f32[H][W].
 *   _device borrows images that are already resident (rgb_pixel_stride 3, or 4 for an RGBA image whose
 *   alpha is ignored).  tf_keyframe_set_pose: f32(SE3d.inverse().matrix()) of Frame::pose_sophus[0],
 *   16 floats row-major (Patch.cpp:51) -- poses move with every bundle adjustment, so it is set before
 *   GeneratePatches. */
TF_API int tf_keyframe_cache(tf_volume* v, int32_t kf_id, const uint8_t* rgb, const float* depth);
TF_API int tf_keyframe_cache_device(tf_volume* v, int32_t kf_id, const uint8_t* d_rgb, int32_t rgb_pixel_stride,
                                    const float* d_depth);
TF_API int tf_keyframe_set_pose(tf_volume* v, int32_t kf_id, const float pose_inv16[16]);
TF_API int tf_keyframe_release(tf_volume* v, int32_t kf_id);
/* Atlas::SetResolution  Structure/Atlas.h:62-65 */
TF_API int tf_atlas_patch_size(tf_volume* v, int32_t* patch_w, int32_t* patch_h);
/* Atlas::loc_next */
TF_API int tf_atlas_loc_next(tf_volume* v, uint64_t* loc_next);
/* MAX_PATCH_WIDTH x MAX_PATCH_HEIGHT of this volume's texture_buffer (Structure/Atlas.h:29-30; tf_config.atlas_w / _h) */
TF_API int tf_atlas_size(tf_volume* v, int32_t* atlas_w, int32_t* atlas_h);
/* ChunkManager::allMeshes[id] = a mesh built by the caller (a host that keeps its own mesher): Mesh::vertices /
 *   normals / colors as 3 f32 per vertex, Mesh::indices, packed by running offsets; creates missing chunks. */
TF_API int tf_meshes_upload(tf_volume* v, const int32_t* ids, int64_t n, const int64_t* vert_offsets,
                            const int64_t* index_offsets, const float* verts, const float* normals,
                            const float* colors, const uint32_t* indices);
/* Chisel::GeneratePatches(chunksToUpdate, labelset, frame_list, camera)  Structure/Chisel.cpp:149-189: for the
 *   listed chunks that have a mesh, in list order: Atlas::AddPatch (first call hands out the next slot,
 *   Atlas.cpp:43-64; later calls keep it, Patch::clear) -> Patch::CalculateTexCoords in keyframe labels[i]
 *   (Patch.cpp:40-108) -> SetFrameid / SetImage.  out_hot = atlas.hot_start / hot_end.
 *   Returns TF_ERR_ATLAS_FULL when the atlas overflows (GeneratePatches' -1): the entry that did not get a
 *   slot and everything behind it in the list stays unprocessed.
 *   At the image's borders the reference's arithmetic is kept as it is: cameraX >= W clamps to W (not W - 1), x == W
 *   reads the next row's first pixel (cv::Mat::at is unchecked), the bilinear tap kinds are its four.  Undefined
 *   behaviour of the reference, defined here (every entry point that runs this stage, the fused ones included): a
 *   read past the image's last pixel returns 0; an image coordinate that is NOT A NUMBER (0 / 0 for a vertex at the
 *   keyframe's centre, a NaN in the pose or the vertex) counts as outside the image -- the patch is flagged caution
 *   and the coordinate clamps to 0 like a negative one -- so box, texcoords and texcolors are finite and do not
 *   depend on the vertex order (the reference's min / max fold keeps the extremum of the vertices
 *   behind the last NaN, and converts floor(NaN) to int). */
TF_API int tf_generate_patches(tf_volume* v, const int32_t* ids, int64_t n, const int32_t* labels,
                               uint64_t out_hot[2]);
/* Chisel::GeneratePatches with labelset = the resident chunk graph (Structure/Chisel.cpp:156-182, tf_texmap_* above): the
 *   keyframe of entry i is its chunk's resident label, looked up on the device in the keyframe cache (what
 *   tf_generate_patches does on the host per label).  A listed chunk with a mesh that is no node, or whose label names no
 *   cached keyframe: TF_ERR_INVALID; that entry and everything behind it in the list stays unprocessed, as for a full
 *   atlas.  tf_compensate_color reads what this call wrote and nothing tf_update_atlas writes, so calling it behind
 *   tf_update_atlas equals the reference's order (MobileFusion.cpp:374-382). */
TF_API int tf_generate_patches_selected(tf_volume* v, const int32_t* ids, int64_t n, uint64_t out_hot[2]);
/* Chisel::CompensateColor()  Structure/Chisel.cpp:198-286 (+ computeMeanAndCov, Structure/Patch.cpp:342-348)
 *   over every mesh with a patch, in ascending chunk-id order (the reference iterates an unordered_map).
 *   Patches with has_adjusted are skipped; the rest is clustered by frame id (cluster order = first
 *   appearance).  Per cluster: mean / covariance of texcolor and of the mesh colours over the patches without
 *   wrong_mapping, the 3x3 transfer T, labs[k] = T (texcolor[k] - mean_src) + mean_tar, has_adjusted = 1.
 *   Reductions and the per-vertex transfer run on the device, the 3x3 eigen-decompositions on the host (f64
 *   Jacobi; Eigen's own iteration is not restated, the result agrees to float rounding). */
TF_API int tf_compensate_color(tf_volume* v, int64_t* out_n_clusters);
/* Chisel::CompensateColor (Structure/Chisel.cpp:198-286) with nothing crossing to the host: asynchronous on the
 * handle's stream.  d_n_clusters (device memory, may be NULL) receives the cluster count.
 *   The semantics are tf_compensate_color's: every mesh of the map that has a patch takes part, patches with has_adjusted
 *   are skipped, the rest is clustered by frame id; a cluster whose patches all map wrongly learns nothing (has_adjusted
 *   stays clear) and still counts; wrongly mapped patches of a learnt cluster get has_adjusted and no labs.  The list of
 *   patches, the clusters, both reductions, the two 3x3 eigen-decompositions per cluster (the same f64 Jacobi text as the
 *   host path's, tf_cc_solve.h) and the transfer run as kernels; the call returns when they are enqueued.  Sums are
 *   accumulated in f64 in an order that depends on the set of patches only (ascending chunk key, vertex index): two runs
 *   over the same map give the same bits; against tf_compensate_color (f32 trees) labs agree to float rounding.
 *   Its buffers (about 230 B per tf_config.max_chunks) are allocated by the first call and freed by tf_volume_reset /
 *   tf_volume_destroy; a handle that never calls it (or the tail with TF_TAIL_COMPENSATE_COLOR) holds none. */
TF_API int tf_compensate_color_device(tf_volume* v, uint32_t* d_n_clusters);
/* tf_compensate_color_device with a device word of the handle's own as d_n_clusters, then tf_sync and that word read
 *   back into *out_n_clusters: for callers (and tests) that want the count on the host and accept the wait. */
TF_API int tf_compensate_color_device_count(tf_volume* v, int64_t* out_n_clusters);
/* Chisel::UpdateAtlas(chunksToUpdate)  Structure/Chisel.cpp:191-196 -> Atlas::UpdateBuffer (Atlas.cpp:71-91):
 *   the keyframe ROI of every listed complete() patch is copied -- or cv::resize'd when it exceeds the slot --
 *   into the atlas. */
TF_API int tf_update_atlas(tf_volume* v, const int32_t* ids, int64_t n);
/* Chisel::DrawMeshes  Structure/Chisel.cpp:288-355: the interleaved vertex stream the renderer / exporter
 *   consumes, 12 f32 per vertex
 *     [x, y, z, 50, (float)(R<<16|G<<8|B), adj, u/atlas_w, v/atlas_h, nx, ny, nz, wrong_mapping]
 *   with (u,v) = texcoord * (ratio < 1 ? ratio : 1) + slot origin (Atlas::GetTexLoc) and
 *   adj = has_adjusted && !labs.empty() ? (float)(3 x 9 bit of int((labs - texcolor) * 255) + 255) : 0, plus
 *   the index stream rebased by the running vertex count, over every mesh whose patch is complete()
 *   (Patch.cpp:191-196), in ascending chunk-id order.  _device leaves both streams in HBM (e.g. a mapped GL
 *   buffer, MobileFusion.h:404-446).
 *   Undefined in the reference, defined here: a colour delta labs - texcolor that is not a number -- the labs of
 *   a cluster of one vertex, whose covariance is 0 / (N - 1) = 0 / 0 while has_adjusted is set all the same --
 *   packs as a zero delta, 255 in its 9-bit field; the other fields of the vertex keep their values. */
TF_API int tf_draw_meshes(tf_volume* v, float* vertices, uint32_t* indices, int64_t cap_vertices,
                          int64_t cap_indices, int64_t* n_vertices, int64_t* n_indices);
TF_API int tf_draw_meshes_device(tf_volume* v, float* d_vertices, uint32_t* d_indices, int64_t cap_vertices,
                                 int64_t cap_indices, int64_t* n_vertices, int64_t* n_indices);
/* ---- rendering the textured model from a pose (tf_render.hip) -----------------------------
 * What the reference's GL viewer does with DrawMeshes' stream and the atlas (GCFusion/MobileFusion.h:404-476,
 * Shaders/draw_mesh.vert / .frag), as a software rasteriser on the device.  These calls only read: the vertex / index
 * stream, the texture or the atlas.  No voxel, hash entry, dirty mark, mesh-filter summary, neighbour-table word or
 * statistic changes, and neither does a mesh, a patch or an atlas texel.  A handle renders its own meshes, as it
 * raycasts its own chunks; there is no multi-rank render.
 *
 * Inputs: vertices f32[n_vertices][12] exactly as tf_draw_meshes writes them (col 3 is not read), indices
 * u32[n_indices] (n_indices % 3 == 0), a texture u8[tex_h][tex_w][3] (NULL = the handle's atlas), the camera tf_raycast
 * would use (tf_raycast_camera, else tf_set_camera; int-truncated intrinsics), pose = camera-to-world 3x4, 0 <= near <
 * far, mode = the reference's colorType: 1 colour = -normal, 2 vertex colour, 3 texture + the interpolated 9-bit colour
 * delta, 4 texture only (3 and 4: a triangle whose first vertex has wrong_mapping takes mode 2's colour; a vertex with
 * adj == 0 decodes to a delta of -1 per channel, as in the reference, so patches without labs are black in mode 3).
 * A vertex projects to sx = fx x / z + cx + 0.5 (sy likewise) and pixel (x, y) is sampled at (sx, sy) = (x, y): the ray
 * tf_raycast casts for that pixel.  Coordinates snap to 1 / 256 pixel, coverage is decided in integers with the
 * top-left rule (two triangles sharing an edge cover each sample on it once), depth and attributes are
 * perspective-correct, the nearest fragment wins and the lower triangle on equal depth; texture sampling is bilinear,
 * clamped to the edge, one level.  No clipping: a triangle is dropped whole when an index is >= n_vertices, a camera
 * coordinate is not finite, a vertex lies in front of near, a snapped coordinate lies beyond +-16384 pixels or its
 * snapped area is 0; a fragment outside [near, far] is discarded.  No back-face culling, no mip maps, no anti-aliasing,
 * no Phong mode.  Two runs give the same bits.  Order of operations: tf_render.hip, restated in tests/render_ref.py.
 * Outputs, each W x H of the camera active at the call, NULL = not written, at least one: rgba u8[H][W][4] (a = 255
 * where covered, 0 0 0 0 where empty), depth f32[H][W] camera-frame z (0 = empty), tri i32[H][W] index position / 3 of
 * the winning triangle (-1 = empty).
 * d_rgba must be 4-byte aligned (it is written one pixel, four bytes, at a time), d_depth and d_tri as their types ask;
 * memory from hipMalloc is.
 * TF_ERR_INVALID: mode outside 1..4, n_indices % 3 != 0, near / far not 0 <= near < far < inf, no camera (a handle is
 * created with one, so: intrinsics that truncate to 0), no output, a texture of no size in modes 3 / 4 with an rgba
 * output.  (tf_volume_create allocates the atlas, so "no atlas" cannot occur through this header; the library still
 * checks the pointer.)
 * tf_render_stream_device: everything in device memory, asynchronous on the handle's stream (the key buffer, 8 bytes per
 * pixel, and the queue of large triangles live in the handle's scratch pool, which waits for the device only when it
 * has to grow).  tf_render_stream: host arrays staged through the pool, synchronous. */
TF_API int tf_render_stream_device(tf_volume* v, const float* d_vertices, int64_t n_vertices, const uint32_t* d_indices,
                                   int64_t n_indices, const uint8_t* d_texture, int32_t tex_w, int32_t tex_h,
                                   const float pose[12], float near_plane, float far_plane, int32_t mode, uint8_t* d_rgba,
                                   float* d_depth, int32_t* d_tri);
TF_API int tf_render_stream(tf_volume* v, const float* vertices, int64_t n_vertices, const uint32_t* indices,
                            int64_t n_indices, const uint8_t* texture, int32_t tex_w, int32_t tex_h, const float pose[12],
                            float near_plane, float far_plane, int32_t mode, uint8_t* rgba, float* depth, int32_t* tri);
/* The current model, rendered with the atlas: the stream is the handle's resident model stream (tf_model_stream_* below).
 * While that stream is current -- packed since the last call that could have changed a mesh, a patch or a pool slot --
 * a render packs nothing and waits for nothing: tf_render_model_device is then asynchronous like tf_render_stream_device,
 * and where the host has not read the stream's counts the rasteriser takes them from the stream's control block (grids
 * and the queue of large triangles are sized from the capacity, surplus lanes leave at once).  While it is not, the render
 * first packs it as tf_model_stream_update does: one wait.  Atlas texels are read at render time and are no part of the
 * stream.  A model with no complete() patch renders an empty image and returns 0.
 * A render behind a tf_model_stream_update_device whose model did not fit is such a render too: that stream counts as
 * current, its control block reads 0 vertices, so the image is EMPTY (the previous model still lies in the buffers but is
 * not shown) until the next synchronising call reports TF_ERR_CAPACITY and the caller reserves more or calls
 * tf_model_stream_update.  tf_model_stream_stats counts that render as served from the stream all the same.
 * Memory: the first render (or tf_model_stream_* call) of a handle allocates the pack's lists, about 84 B per
 * tf_config.max_chunks (44 MB at 2^19 chunks), and, where nothing was reserved, a stream of 2^16 vertices / 3 * 2^16
 * indices (3.9 MB) even for an empty model -- earlier a render allocated the stream alone.  tf_model_stream_release
 * gives all of it back. */
TF_API int tf_render_model_device(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t mode,
                                  uint8_t* d_rgba, float* d_depth, int32_t* d_tri);
TF_API int tf_render_model(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t mode,
                           uint8_t* rgba, float* depth, int32_t* tri);
/* ---- the model stream, resident in the handle (tf_model.hip) -------------------------------
 * Chisel::DrawMeshes (Structure/Chisel.cpp:288-355; GCFusion/MobileFusion.cpp:384 at the end of a keyframe) into buffers
 * of the handle's own, with nothing crossing to the host: the list of complete() patches, their order (ascending chunk
 * id, as tf_draw_meshes), the running vertex / index counts and the pack are kernels on the handle's stream, the counts
 * stay in device words.  The contents are tf_draw_meshes' bit for bit (the same text per patch).  The stream is kept
 * until the model changes: the handle counts a model generation that EVERY entry point advances except a named set of
 * readers -- tf_model_stream_*, tf_render_*, tf_raycast*, tf_query_points*, tf_sync, and the getters that touch no
 * device state (tf_atlas_size, tf_atlas_patch_size, tf_atlas_snapshot_rows, tf_last_error) -- so a reader missing from
 * that set costs one repack and no writer can be missed; a reader that first has to bring deferred frames onto the
 * stream counts as a writer for that call.  A stream is current when it was packed at the present generation.
 *   control block  u32[8] {n_vertices, n_indices, n_patches, status, need_vertices, need_indices, 0, 0}: status != 0 = the
 *                  model did not fit; then n_* are 0, need_* say what it takes, and NOTHING was written -- the buffers
 *                  hold what they held, a half-written model is never visible.  (need_* are always what the model takes.)
 *   tf_model_stream_reserve        sets the capacity in vertices / indices (the reference's tsdf_vertices_buffer /
 *                  tsdf_indices_buffer are fixed-size too).  A changed capacity reallocates (waits for the stream once)
 *                  and drops the contents; it never goes below what a current stream holds.
 *   tf_model_stream_update_device  enqueues the pack and returns: no wait, no copy to the host.  TF_ERR_INVALID without a
 *                  capacity (tf_model_stream_reserve, or one left by tf_model_stream_update / tf_render_model).  A
 *                  model that does not fit sets a sticky status bit: the next synchronising call returns
 *                  TF_ERR_CAPACITY, as for a full mesh store.  Behind tf_texture_tail_device this is the reference's
 *                  DrawMeshes at MobileFusion.cpp:384, and the keyframe still waits once.
 *   tf_model_stream_update         the same, then one wait for the control block; on overflow the buffers grow to a power
 *                  of two (at least 2^16 vertices / 3 * 2^16 indices) and the pack runs again; nothing becomes sticky.
 *                  Counts returned (either may be NULL); a model with no complete() patch gives 0 / 0 and TF_OK.
 *   tf_model_stream_get            borrows the device pointers (any may be NULL); d_counts is the control block.  Valid until a
 *                  call that reallocates or frees the buffers (reserve with another capacity, a growing update /
 *                  render, release, tf_volume_reset, tf_volume_destroy).  Does not synchronise: order reads behind the
 *                  handle's stream.  TF_ERR_INVALID while there are no buffers.
 *   tf_model_stream_stats          host counters, no wait: out[0] packs enqueued, out[1] tf_render_model(_device) calls
 *                  served from a current stream without a pack, out[2] / out[3] capacity in vertices / indices.
 *   tf_model_stream_release        waits for the stream, frees the buffers (about 84 B per tf_config.max_chunks besides the
 *                  two streams); tf_volume_reset and tf_volume_destroy do the same.  The counters stay.
 *   tf_model_stream_time           measurement aid, no part of the flow: one pack between HIP events on the handle's stream,
 *                  then a wait; us[0..3] = list, rank (with the placing), scan, write in microseconds (tools/model_stream_time.py).  It is
 *                  an entry point of its own, like tf_profile_calibrate, because tf_profile's kinds are a fixed-size
 *                  part of the ABI (TF_PROF_COUNT) that four more kinds would change for every caller.  Needs a
 *                  capacity (TF_ERR_INVALID without); a model that does not fit is timed as it is and raises NO sticky
 *                  status. */
TF_API int tf_model_stream_reserve(tf_volume* v, int64_t cap_vertices, int64_t cap_indices);
TF_API int tf_model_stream_update_device(tf_volume* v);
TF_API int tf_model_stream_update(tf_volume* v, int64_t* n_vertices, int64_t* n_indices);
TF_API int tf_model_stream_get(tf_volume* v, const float** d_vertices, const uint32_t** d_indices,
                               const uint32_t** d_counts, int64_t* cap_vertices, int64_t* cap_indices);
TF_API int tf_model_stream_stats(tf_volume* v, int64_t out[4]);
TF_API int tf_model_stream_release(tf_volume* v);
TF_API int tf_model_stream_time(tf_volume* v, double us[4]);
/* Patch mirrors of listed chunks (Structure/Patch.h:51-94): texloc (~0 = no slot), frameid, boundingbox
 *   (x, y, w, h), flags (TF_PATCH_*), ratio; texcoord f32[2 nv], texcolor / labs f32[3 nv] packed by
 *   vert_offsets (from tf_mesh_counts).  Any output may be NULL. */
#define TF_PATCH_HAS_PATCH 1      /* Mesh::m_patch != nullptr */
#define TF_PATCH_CAUTION 2        /* CalculateTexCoords returned -1 */
#define TF_PATCH_WRONG_MAPPING 4  /* Patch::wrong_mapping */
#define TF_PATCH_HAS_IMAGE 8      /* Patch::has_image */
#define TF_PATCH_HAS_ADJUSTED 16  /* Patch::has_adjusted */
TF_API int tf_patches_download(tf_volume* v, const int32_t* ids, int64_t n, const int64_t* vert_offsets,
                               uint64_t* texloc, int32_t* frameid, int32_t* bbox, int32_t* flags, float* ratio,
                               float* texcoord, float* texcolor, float* labs);
/* Atlas::texture_buffer rows [row0,row1) (MobileFusion.h:406-421 uploads the hot rows) */
TF_API int tf_atlas_download_rows(tf_volume* v, int64_t row0, int64_t row1, uint8_t* dst);
/* The same rows for a thread OTHER than the one that drives the handle -- the reference's GUI thread reads
 *   atlas.texture_buffer while the map thread writes it (GCFusion/MobileFusion.h:404-421; SURVEY.md s.8(b) "Threading").
 *   tf_atlas_download_rows belongs to the driving thread: like every entry point it first brings the handle's deferred work
 *   onto the stream.  This one touches no state of the pipeline and may run at any time next to the driving thread's calls:
 *   the rows are copied device-to-device INSIDE the handle's stream, between two of the driving thread's launches, so they
 *   show ONE moment of the stream -- every atlas write enqueued before it, none enqueued after it -- and travel to dst on a
 *   stream of the reader's own.  *write_seq = atlas-writing launches ahead of the snapshot (monotonic), *frame_id = the
 *   label (Patch::frameid) of the newest fused frame among them, -1 = none yet; both may be NULL.  Concurrent readers are
 *   serialised. */
TF_API int tf_atlas_snapshot_rows(tf_volume* v, int64_t row0, int64_t row1, uint8_t* dst, int64_t* write_seq, int32_t* frame_id);

/* ---- frame pre-processing that feeds the path ---------------------------------
 * The per-frame image passes main.cpp:117-147 runs before a frame reaches the fusion path, on images resident in
 * device memory (row-major f32 depth / weight / quality, PLANAR f32 normal maps [3][H][W], packed u8 RGB), with the
 * untruncated intrinsics given to tf_set_camera (the reference passes camera.c_fx ...).  Asynchronous on the
 * handle's stream except tf_pre_refine_keyframe.  Pixels the reference leaves uninitialised are written as 0;
 * _mm256_rsqrt_ps is the correctly rounded 1 / sqrt (see oracle/tf_oracle.c).
 *   tf_pre_frame_depth           DatasetWrapper::framePreprocess     Tools/DatasetWrapper.hpp:186-263 (see below)
 *   tf_pre_normal_map            BasicAPI::extractNormalMapSIMD      BasicAPI.cpp:849-905
 *   tf_pre_refine_depth_normal   BasicAPI::refineDepthUseNormalSIMD  BasicAPI.cpp:728-781   (normal, depth in place)
 *   tf_pre_color_valid           BasicAPI::checkColorQuality         BasicAPI.cpp:783-806   (Frame::colorValidFlag)
 *   tf_pre_color_quality         BasicAPI::estimateColorQuality      BasicAPI.cpp:815-847   (Frame::observationQualityMap)
 *   tf_pre_refine_newframe       BasicAPI::refineNewframesSIMD       BasicAPI.cpp:378-443   (depth_new in place;
 *                                T = f32 of (pose_ref^-1 * pose_new).matrix()[3x4], row-major)
 *   tf_pre_refine_keyframe       BasicAPI::refineKeyframesSIMD       BasicAPI.cpp:506-636   (depth_ref, weight_ref in
 *                                place with the reference's sequential in-place semantics; T = f32 of
 *                                (pose_new^-1 * pose_ref).matrix()[3x4]; synchronises)
 * The two refinement passes return TF_ERR_INVALID when the width is not a multiple of 8: the reference's 8-pixel
 *   groups run over the row end there and have no result to match (tf_set_camera takes no such width either).
 * tf_pre_refine_keyframe reaches the sequential in-place result as a fixed point, one link of the dependency chain
 *   per round, for any chain the image can hold: a keyframe fresh from the loader (weight 0) can take one round per
 *   image row, and no image takes more than W * H / 8 + 1.  Rounds are queued in growing batches and the iteration
 *   stops at the first batch whose last round changed nothing, so *rounds (may be NULL) = ROUNDS RUN, which can
 *   exceed the chain length.  On every error return d_depth_ref and d_weight_ref are untouched. */
/* DatasetWrapper::framePreprocess (Tools/DatasetWrapper.hpp:186-263, the loader's depth pass ahead of all of the
 *   above): raw u16 depth (device, updated in place like Frame::depth) -> readings above maximum_depth * depth_scale
 *   dropped -> metres -> cv::bilateralFilter(refined_depth, ., d = 9 (7 on MobileCPU builds), sigma_color = 0.03,
 *   sigma_space = 10) -> d_refined (Frame::refined_depth, f32, may be NULL) and written back to the u16 map.  The
 *   filter restates OpenCV's CV_32FC1 algorithm (4096-bin colour table over the image's own range, circular taps,
 *   BORDER_REFLECT_101); tap sums run in tap order, which OpenCV's vector builds do not pin (oracle/tf_oracle.c).
 *   Asynchronous on the handle's stream; d <= 15. */
TF_API int tf_pre_frame_depth(tf_volume* v, uint16_t* d_depth, float* d_refined, float maximum_depth, float depth_scale,
                              int d, double sigma_color, double sigma_space);
TF_API int tf_pre_normal_map(tf_volume* v, const float* d_depth, float* d_normal);
TF_API int tf_pre_refine_depth_normal(tf_volume* v, float* d_normal, float* d_depth);
TF_API int tf_pre_color_valid(tf_volume* v, const float* d_normal, uint8_t* d_flag);
TF_API int tf_pre_color_quality(tf_volume* v, const float* d_depth, const float* d_normal, const uint8_t* d_rgb,
                                float* d_quality);
TF_API int tf_pre_refine_newframe(tf_volume* v, const float* d_depth_ref, float* d_depth_new,
                                  const float T_new_to_ref[12]);
TF_API int tf_pre_refine_keyframe(tf_volume* v, float* d_depth_ref, float* d_weight_ref, const float* d_depth_new,
                                  const float T_ref_to_new[12], int32_t* rounds);

#ifdef __cplusplus
}
#endif
#endif /* TF_FUSION_H_ */
