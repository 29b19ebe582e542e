// The reference's tail of MobileFusion::tsdfFusion (GCFusion/MobileFusion.cpp:345-382) through the host mirror
// (texturefusion_amd/host/tf_chisel.hpp) on a synthetic room: per keyframe the keyframe unit without its texture stage,
// CompressMeshes, TexMap::update_chunkgraph_device / update_datacost_device (/ check_graph when a keyframe moved),
// TexMap::view_selection(kflist) -- the solve on the device --, GeneratePatches with the graph's labels, UpdateAtlas.
// Checked after every keyframe:
//   every node's label is a keyframe that observes it, or what the label-0 rule gives (TexMap.cpp:238-242);
//   the reported energy is the energy of the graph's labels (recomputed here in f64) and is not above the energy of the
//   labelling that gives every chunk its best-quality keyframe;
//   view_selection(chunksToUpdate, kflist) changes labels only inside `concerns`;
//   the patches' frameid equal the labels.
// Built and run by tests/test_gpu_view_selection.py, which writes the frames (argv[1]); prints "mirror ok ..." and exits 0.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

extern "C" {
int hipMalloc(void** p, size_t n);
int hipFree(void* p);
int hipMemcpy(void* dst, const void* src, size_t n, int kind);
}

#define REQUIRE(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct HostFrame {
  float pose[12], pose_inv[16];
  void *d_depth = nullptr, *d_rgba = nullptr, *d_quality = nullptr;
};

static void* upload(const void* src, size_t n) {
  void* p = nullptr;
  if (hipMalloc(&p, n) != 0 || hipMemcpy(p, src, n, 1) != 0) { std::printf("hip upload failed\n"); std::exit(2); }
  return p;
}

// unary of row r of a non-empty column, as TexMap.cpp:168-175
static float unary(const SparseMat::Column& col, std::size_t r) {
  float column_max = col.begin()->second;
  for (const auto& e : col) if (column_max < e.second) column_max = e.second;
  return 1.0f - col.at(r) / column_max;
}

// f64 energy of a row choice per node (rows[i] ignored for nodes with an empty column: cost 1, no edges)
static double energy(const TexMap& tex, const std::vector<std::size_t>& rows) {
  const std::size_t n = tex.chunkGraph.num_nodes();
  auto empty = [&](std::size_t k) { return k >= tex.dataCost.cols() || tex.dataCost.col(k).empty(); };
  double e = 0.0;
  for (std::size_t i = 0; i < n; ++i) {
    if (empty(i)) { e += 1.0; continue; }
    e += (double)unary(tex.dataCost.col(i), rows[i]);
    for (std::size_t adj : tex.chunkGraph.get_adj_nodes(i))
      if (i < adj && !empty(adj) && rows[i] != rows[adj]) e += (double)(tex.adjacent_cost * tex.pairwise_cost);
  }
  return e;
}

int main(int argc, char** argv) {
  REQUIRE(argc == 2, "usage: mirror_view_selection <frames file>");
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f, "cannot open %s", argv[1]);
  int32_t hd[3];
  float cam[7];
  REQUIRE(std::fread(hd, 4, 3, f) == 3 && std::fread(cam, 4, 7, f) == 7, "header");
  const int n_frames = hd[0], W = hd[1], H = hd[2];
  const size_t P = (size_t)W * H;
  std::vector<HostFrame> fr((size_t)n_frames);
  {
    std::vector<float> depth(P), quality(P);
    std::vector<uint8_t> rgba(4 * P);
    for (auto& x : fr) {
      REQUIRE(std::fread(x.pose, 4, 12, f) == 12 && std::fread(x.pose_inv, 4, 16, f) == 16 &&
              std::fread(depth.data(), 4, P, f) == P && std::fread(rgba.data(), 1, 4 * P, f) == 4 * P &&
              std::fread(quality.data(), 4, P, f) == P, "frame");
      x.d_depth = upload(depth.data(), 4 * P);
      x.d_rgba = upload(rgba.data(), 4 * P);
      x.d_quality = upload(quality.data(), 4 * P);
    }
  }
  std::fclose(f);

  tf_config cfg = {};
  cfg.max_chunks = 1 << 16;
  const int chunkSize[3] = {8, 8, 8};
  chisel::Chisel ch(chunkSize, cam[6], true, &cfg);
  tf_volume* v = ch.Handle();
  chisel::tf_check(tf_set_camera(v, cam[0], cam[1], cam[2], cam[3], W, H, cam[4], cam[5]), "camera");

  struct Step { int kf_id, key; std::vector<int> local; bool move_first; };
  const std::vector<Step> plan = {{4, 0, {1, 2, 3, 4}, false}, {9, 5, {6, 7, 8, 9, 10}, false}, {13, 11, {12, 13}, true}, {14, 14, {15}, false}};
  REQUIRE(n_frames >= 16, "16 frames needed");
  auto fill = [&](tf_unit_group& g, const Step& s, int shift) {  // shift: every frame takes the pose of the frame `shift` further on
    std::memset(&g, 0, sizeof g);
    g.kf_id = s.kf_id;
    g.n_local = (int32_t)s.local.size();
    g.keyframe.d_depth = (const float*)fr[(size_t)s.key].d_depth;
    g.keyframe.d_rgba = (const uint8_t*)fr[(size_t)s.key].d_rgba;
    g.keyframe.d_quality = (const float*)fr[(size_t)s.key].d_quality;
    std::memcpy(g.keyframe.pose, fr[(size_t)(s.key + shift)].pose, 48);
    for (size_t i = 0; i < s.local.size(); ++i) {
      g.local[i].d_depth = (const float*)fr[(size_t)s.local[i]].d_depth;
      std::memcpy(g.local[i].pose, fr[(size_t)(s.local[i] + shift)].pose, 48);
    }
  };

  TexMap tex;
  std::vector<MultiViewGeometry::KeyFrameDatabase> kflist;
  std::vector<int> lookup(32, -1);
  long checked = 0, relabelled = 0, unlabelled = 0, sub_changed = 0, all_patches = 0, solves = 0;
  for (size_t s = 0; s < plan.size(); ++s) {
    const Step& st = plan[s];
    // kflist: the keyframes integrated so far and the newest one, which is not integrated yet (tsdfFusion integrates
    // kflist[integrateKeyframeID], the keyframe before the newest: kflist[size - 2] is the one this step integrates)
    if (kflist.empty()) { kflist.emplace_back(); kflist.back().keyFrameIndex = st.kf_id; }
    lookup[(size_t)st.kf_id] = (int)kflist.size() - 1;
    kflist.emplace_back();
    kflist.back().keyFrameIndex = s + 1 < plan.size() ? plan[s + 1].kf_id : 16;
    tf_unit_group fresh, moved;
    fill(fresh, st, 0);
    std::memset(&moved, 0, sizeof moved);
    std::vector<int> keyframesToUpdate;
    if (st.move_first) {  // a loop closure moved the first keyframe group: each frame to the pose of the next frame
      fill(moved, plan[0], 1);
      std::memcpy(moved.old_keyframe_pose, fr[(size_t)plan[0].key].pose, 48);
      for (size_t i = 0; i < plan[0].local.size(); ++i) std::memcpy(moved.old_local_pose[i], fr[(size_t)plan[0].local[i]].pose, 48);
      keyframesToUpdate.push_back(plan[0].kf_id);
    }
    chisel::tf_check(tf_keyframe_unit_device(v, &fresh, &moved, st.move_first ? 1 : 0, 0, nullptr), "unit");
    std::vector<int32_t> ids(3 << 16);
    int64_t n = 0;
    chisel::tf_check(tf_compress_meshes(v, ids.data(), 1 << 16, &n), "CompressMeshes");
    // (the first groups of the orbit may leave no chunk with a mesh: the flow runs with an empty list, as the reference's would)
    chisel::ChunkIDList chunksToUpdate;
    for (int64_t i = 0; i < n; ++i) chunksToUpdate.emplace_back(ids[3 * (size_t)i], ids[3 * (size_t)i + 1], ids[3 * (size_t)i + 2]);
    chisel::tf_check(tex.update_chunkgraph_device(chunksToUpdate, v), "update_chunkgraph");
    chisel::tf_check(tex.update_datacost_device(chunksToUpdate, v, lookup, st.kf_id, keyframesToUpdate), "update_datacost");
    if (!keyframesToUpdate.empty()) {  // MobileFusion.cpp:360-361
      std::vector<int32_t> mids(3 << 16);
      int64_t nm = 0;
      chisel::tf_check(tf_list_meshes(v, mids.data(), 1 << 16, &nm), "list meshes");
      mids.resize((size_t)nm * 3);
      ch.chunkManager.RefreshMeshes(mids);
      tex.check_graph(ch.chunkManager);
    }
    // the keyframes the labels can name are cached, the moved one with its new pose
    const HostFrame& key = fr[(size_t)st.key];
    chisel::tf_check(tf_keyframe_cache_device(v, st.kf_id, (const uint8_t*)key.d_rgba, 4, (const float*)key.d_depth), "cache");
    chisel::tf_check(tf_keyframe_set_pose(v, st.kf_id, key.pose_inv), "pose");
    if (st.move_first) chisel::tf_check(tf_keyframe_set_pose(v, plan[0].kf_id, fr[(size_t)plan[0].key + 1].pose_inv), "moved pose");
    const std::size_t N = tex.chunkGraph.num_nodes();
    if (N == 0) continue;  // MobileFusion.cpp:362
    const std::vector<int> before = tex.chunkGraph.labels;
    tex.view_selection(kflist);
    ++solves;
    REQUIRE(tex.labelstorage.size() == N && tex.solved_labels.size() == N, "labelstorage");
    REQUIRE(tex.energy_trace.size() >= 2 && tex.energy_trace.size() <= 32, "did not converge: %zu rounds", tex.energy_trace.size() - 1);
    for (size_t r = 1; r < tex.energy_trace.size(); ++r) REQUIRE(tex.energy_trace[r] <= tex.energy_trace[r - 1], "energy rose in round %zu", r);
    // labels: an observing keyframe, or the label-0 rule
    std::vector<std::size_t> rows(N, 0), best(N, 0);
    for (std::size_t i = 0; i < N; ++i) {
      const int label = tex.chunkGraph.get_label(i);
      const bool none = i >= tex.dataCost.cols() || tex.dataCost.col(i).empty();
      if (none) {
        const int prev = i < before.size() ? before[i] : 0;
        REQUIRE(label == (prev != 0 ? prev : kflist[kflist.size() - 2].keyFrameIndex), "node %zu: label %d, was %d", i, label, prev);
        REQUIRE(tex.labelstorage[i] == 0, "node %zu: stored label %d", i, tex.labelstorage[i]);
        ++unlabelled;
      } else {
        REQUIRE(label >= 0 && label < (int)lookup.size() && lookup[(size_t)label] >= 0, "node %zu: label %d is no keyframe", i, label);
        rows[i] = (std::size_t)lookup[(size_t)label];
        const SparseMat::Column& col = tex.dataCost.col(i);
        REQUIRE(col.count(rows[i]) == 1, "node %zu: keyframe %d does not observe it", i, label);
        REQUIRE(tex.labelstorage[i] == (int)rows[i] + 1, "node %zu: stored label", i);
        best[i] = col.begin()->first;
        for (const auto& e : col) if (e.second > col.at(best[i])) best[i] = e.first;
        relabelled += i < before.size() && before[i] != label;
      }
      ++checked;
    }
    const double e_final = energy(tex, rows), e_best = energy(tex, best);
    std::printf("keyframe %d: %zu nodes, %zu edges, %zu rounds, energy %.9g -> %.9g (best-quality labelling %.9g)\n", st.kf_id, N,
                tex.chunkGraph.num_edges(), tex.energy_trace.size() - 1, tex.energy_trace.front(), tex.energy_trace.back(), e_best);
    REQUIRE(e_final == tex.energy_trace.back(), "reported energy %.17g, labels have %.17g", tex.energy_trace.back(), e_final);
    REQUIRE(e_final <= e_best, "energy %.17g above the best-quality labelling's %.17g", e_final, e_best);

    // GeneratePatches with the graph's labels, UpdateAtlas (Chisel.cpp:149-196)
    std::vector<int32_t> labels((size_t)n);
    for (int64_t i = 0; i < n; ++i) labels[(size_t)i] = tex.chunkGraph.get_label(tex.chunkGraph.chunks.find(chunksToUpdate[(size_t)i])->second);
    uint64_t hot[2] = {0, 0};
    chisel::tf_check(tf_generate_patches(v, ids.data(), n, labels.data(), hot), "GeneratePatches");
    chisel::tf_check(tf_update_atlas(v, ids.data(), n), "UpdateAtlas");
    long patches = 0;
    for (int64_t i = 0; i < n; ++i) {
      int32_t frameid = -1, flags = 0;
      const int rc = tf_patches_download(v, &ids[3 * (size_t)i], 1, nullptr, nullptr, &frameid, nullptr, &flags, nullptr, nullptr, nullptr, nullptr);
      if (rc == TF_ERR_MISSING_CHUNK) continue;
      chisel::tf_check(rc, "patches");
      if (!(flags & TF_PATCH_HAS_PATCH)) continue;
      REQUIRE(frameid == labels[(size_t)i], "patch %lld: frameid %d, label %d", (long long)i, frameid, labels[(size_t)i]);
      ++patches;
    }
    all_patches += patches;

    // the second overload: the sub-problem over a part of chunksToUpdate leaves every other node alone
    chisel::ChunkIDList part;
    std::set<std::size_t> concerns;
    for (int64_t i = 0; i < n; i += 3) {
      part.push_back(chunksToUpdate[(size_t)i]);
      concerns.insert(tex.chunkGraph.chunks.find(part.back())->second);
    }
    part.emplace_back(9999, 9999, 9999);  // (not a node: skipped)
    const std::vector<int> mid = tex.chunkGraph.labels, stored = tex.labelstorage;
    tex.view_selection(part, kflist);
    REQUIRE(tex.solved_labels.size() == concerns.size(), "sub-problem size");
    REQUIRE(tex.labelstorage == stored, "the sub-problem touched labelstorage");
    for (std::size_t i = 0; i < N; ++i) {
      if (concerns.count(i)) { sub_changed += mid[i] != tex.chunkGraph.get_label(i); continue; }
      REQUIRE(mid[i] == tex.chunkGraph.get_label(i), "node %zu outside concerns changed its label", i);
    }
    tex.chunkGraph.labels = mid;  // (the flow goes on from the full solve)
  }
  chisel::tf_check(tf_sync(v), "sync");
  REQUIRE(solves >= 2 && checked > 100 && all_patches > 50, "%ld solves, %ld nodes checked, %ld patches", solves, checked, all_patches);
  REQUIRE(relabelled > 0, "no node was ever relabelled");
  for (auto& x : fr) { hipFree(x.d_depth); hipFree(x.d_rgba); hipFree(x.d_quality); }
  std::printf("mirror ok %ld nodes checked, %ld relabelled, %ld without observation, %ld changed by the sub-problems\n", checked,
              relabelled, unlabelled, sub_changed);
  return 0;
}
