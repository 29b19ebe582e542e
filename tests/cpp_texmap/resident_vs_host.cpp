// The resident TexMap against a yardstick that shares no line with tests/texmap_ref.py: one room sequence driven twice
// through the host mirror (texturefusion_amd/host/tf_chisel.hpp) behind tf_keyframe_unit_device(texture = 0) --
//   run A  update_chunkgraph_device / update_datacost_device / check_graph / view_selection: graph and columns in
//          std::maps on the host, the problem built on the host (TexMap::solve), tf_view_select;
//   run B  the *_resident methods: everything in HBM, the problem assembled on the device;
// and asserts equal chunk labels (by chunk id) and equal f64 traces after every keyframe.
// RetractObservations' data-cost half (MobileFusion.cpp:261-267) for the moved keyframe: run B gets it from the unit
// itself; run A removes row lookup[kf] from every node's column before the unit call, which is the same thing -- an
// entry (chunk, kf) only ever comes from an observation of kf, observations are recorded for updated chunks only, updated
// chunks are in kf.validChunks, and this sequence never deletes a chunk.
#include <cstdio>
#include <cstring>
#include <array>
#include <map>
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
struct Step { int kf_id, key; std::vector<int> local; bool move_first; };
struct Result {
  std::vector<std::map<std::array<int, 3>, int>> labels;  // per keyframe: chunk id -> label
  std::vector<std::vector<double>> traces;
};

static void* upload(const void* src, size_t n) {
  void* p = nullptr;
  if (hipMalloc(&p, n) != 0 || hipMemcpy(p, src, n, 1) != 0) { std::printf("hip upload failed\n"); std::exit(2); }
  return p;
}

static int run(bool resident, const std::vector<HostFrame>& fr, const float* cam, int W, int H, const std::vector<Step>& plan,
               Result& out) {
  tf_config cfg = {};
  cfg.max_chunks = 1 << 16;
  const int chunkSize[3] = {8, 8, 8};
  chisel::Chisel ch(chunkSize, cam[6], true, &cfg);
  tf_volume* v = ch.Handle();
  chisel::tf_check(tf_set_camera(v, cam[0], cam[1], cam[2], cam[3], W, H, cam[4], cam[5]), "camera");
  auto fill = [&](tf_unit_group& g, const Step& s, int shift) {
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
  std::set<std::array<int, 3>> nodes;  // every chunk ever handed to an update: the node set of both runs
  for (size_t s = 0; s < plan.size(); ++s) {
    const Step& st = plan[s];
    if (kflist.empty()) { kflist.emplace_back(); kflist.back().keyFrameIndex = st.kf_id; }
    lookup[(size_t)st.kf_id] = (int)kflist.size() - 1;
    kflist.emplace_back();
    kflist.back().keyFrameIndex = s + 1 < plan.size() ? plan[s + 1].kf_id : 16;
    if (resident) chisel::tf_check(tex.set_keyframes_resident(v, kflist), "set_keyframes");
    tf_unit_group fresh, moved;
    fill(fresh, st, 0);
    std::memset(&moved, 0, sizeof moved);
    std::vector<int> keyframesToUpdate;
    if (st.move_first) {
      fill(moved, plan[0], 1);
      std::memcpy(moved.old_keyframe_pose, fr[(size_t)plan[0].key].pose, 48);
      for (size_t i = 0; i < plan[0].local.size(); ++i) std::memcpy(moved.old_local_pose[i], fr[(size_t)plan[0].local[i]].pose, 48);
      keyframesToUpdate.push_back(plan[0].kf_id);
      if (!resident)
        for (std::size_t k = 0; k < tex.chunkGraph.num_nodes(); ++k) tex.dataCost.remove_observation(k, (std::size_t)lookup[(size_t)plan[0].kf_id]);
    }
    chisel::tf_check(tf_keyframe_unit_device(v, &fresh, &moved, st.move_first ? 1 : 0, 0, nullptr), "unit");
    std::vector<int32_t> ids(3 << 16);
    int64_t n = 0;
    chisel::tf_check(tf_compress_meshes(v, ids.data(), 1 << 16, &n), "CompressMeshes");
    chisel::ChunkIDList chunksToUpdate;
    for (int64_t i = 0; i < n; ++i) {
      chunksToUpdate.emplace_back(ids[3 * (size_t)i], ids[3 * (size_t)i + 1], ids[3 * (size_t)i + 2]);
      nodes.insert({ids[3 * (size_t)i], ids[3 * (size_t)i + 1], ids[3 * (size_t)i + 2]});
    }
    if (resident) {
      chisel::tf_check(tex.update_chunkgraph_resident(chunksToUpdate, v), "update_chunkgraph");
      chisel::tf_check(tex.update_datacost_resident(chunksToUpdate, v, st.kf_id, keyframesToUpdate), "update_datacost");
      if (!keyframesToUpdate.empty()) chisel::tf_check(tex.check_graph_resident(), "check_graph");
    } else {
      chisel::tf_check(tex.update_chunkgraph_device(chunksToUpdate, v), "update_chunkgraph");
      chisel::tf_check(tex.update_datacost_device(chunksToUpdate, v, lookup, st.kf_id, keyframesToUpdate), "update_datacost");
      if (!keyframesToUpdate.empty()) {
        std::vector<int32_t> mids(3 << 16);
        int64_t nm = 0;
        chisel::tf_check(tf_list_meshes(v, mids.data(), 1 << 16, &nm), "list meshes");
        mids.resize((size_t)nm * 3);
        ch.chunkManager.RefreshMeshes(mids);
        tex.check_graph(ch.chunkManager);
      }
    }
    out.labels.emplace_back();
    out.traces.emplace_back();
    if (nodes.empty()) continue;  // MobileFusion.cpp:362
    if (resident) chisel::tf_check(tex.view_selection_resident(), "view_selection");
    else tex.view_selection(kflist);
    out.traces.back() = tex.energy_trace;
    chisel::ChunkIDList all;
    for (const auto& c : nodes) all.emplace_back(c[0], c[1], c[2]);
    std::vector<int32_t> lab;
    if (resident) {
      chisel::tf_check(tex.labels_resident(all, lab), "labels");
    } else {
      REQUIRE(tex.chunkGraph.num_nodes() == nodes.size(), "node sets differ: %zu vs %zu", tex.chunkGraph.num_nodes(), nodes.size());
      for (const auto& c : all) lab.push_back(tex.chunkGraph.get_label(tex.chunkGraph.chunks.find(c)->second));
    }
    size_t k = 0;
    for (const auto& c : nodes) out.labels.back()[c] = lab[k++];
  }
  chisel::tf_check(tf_sync(v), "sync");
  return 0;
}

int main(int argc, char** argv) {
  REQUIRE(argc == 2, "usage: resident_vs_host <frames file>");
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
  REQUIRE(n_frames >= 17, "17 frames needed");
  const std::vector<Step> plan = {{4, 0, {1, 2, 3, 4}, false}, {9, 5, {6, 7, 8, 9, 10}, false}, {13, 11, {12, 13}, true}, {14, 14, {15}, false}};
  Result host, res;
  if (run(false, fr, cam, W, H, plan, host) || run(true, fr, cam, W, H, plan, res)) return 1;
  REQUIRE(host.labels.size() == plan.size() && res.labels.size() == plan.size(), "steps");
  long compared = 0, solves = 0, multi_round = 0;
  for (size_t s = 0; s < plan.size(); ++s) {
    REQUIRE(host.labels[s].size() == res.labels[s].size(), "keyframe %d: %zu vs %zu nodes", plan[s].kf_id, host.labels[s].size(), res.labels[s].size());
    for (const auto& kv : host.labels[s]) {
      const auto it = res.labels[s].find(kv.first);
      REQUIRE(it != res.labels[s].end() && it->second == kv.second, "keyframe %d chunk (%d,%d,%d): host label %d, resident %d", plan[s].kf_id,
              kv.first[0], kv.first[1], kv.first[2], kv.second, it == res.labels[s].end() ? -1 : it->second);
      ++compared;
    }
    REQUIRE(host.traces[s].size() == res.traces[s].size(), "keyframe %d: %zu vs %zu trace entries", plan[s].kf_id, host.traces[s].size(), res.traces[s].size());
    for (size_t r = 0; r < host.traces[s].size(); ++r)
      REQUIRE(host.traces[s][r] == res.traces[s][r], "keyframe %d round %zu: %.17g vs %.17g", plan[s].kf_id, r, host.traces[s][r], res.traces[s][r]);
    solves += !host.traces[s].empty();
    multi_round += host.traces[s].size() > 2;
    std::printf("keyframe %d: %zu nodes, %zu rounds, energy %.9g -> %.9g on both paths\n", plan[s].kf_id, host.labels[s].size(),
                host.traces[s].empty() ? (size_t)0 : host.traces[s].size() - 1, host.traces[s].empty() ? 0.0 : host.traces[s].front(),
                host.traces[s].empty() ? 0.0 : host.traces[s].back());
  }
  REQUIRE(solves >= 2 && compared > 100, "%ld solves, %ld labels compared", solves, compared);
  REQUIRE(multi_round >= 1, "no solve took more than one round: the comparison of the traces would be vacuous");
  for (auto& x : fr) { hipFree(x.d_depth); hipFree(x.d_rgba); hipFree(x.d_quality); }
  std::printf("resident ok %ld labels compared over %ld solves\n", compared, solves);
  return 0;
}
