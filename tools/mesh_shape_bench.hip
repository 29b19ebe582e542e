// What does the memory system give a launch of the mesher's size and access shape, with no marching cubes in it?  One
// 128-thread workgroup per surviving chunk (2929 per S-room frame, ten resident per CU): the chunk's own 4 KiB of
// {sdf, weight}, 410 scattered 16-byte halo loads out of its 26 neighbours' chunks (slots known: no dependent probes),
// everything staged through LDS with one barrier, then 4.2 KB of vertices / triangles written to the chunk's mesh block.
// Two forms of the halo: as round 4 measured it -- a rolled loop whose every turn is slot -> wait -> voxels -> wait -> LDS,
// i.e. up to EIGHT dependent round trips per chunk, which is what the compiler made of the source and not what the
// memory system asks for -- and the batch form of the mesher (LOAD BATCHES): the 27 slots in LDS, then the
// own voxels and every halo load of a thread in flight together, selected behind the wait.
//   hipcc --offload-arch=gfx950 -O3 tools/mesh_shape_bench.hip -o tools/mesh_shape_bench && tools/mesh_shape_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// (granule of halo load k, as the mesher reads the halo: the rules of k_mesh_shape below, as selects -- a load behind a
// lane-dependent branch is waited for on its own)
__device__ __forceinline__ void halo_at(unsigned k, unsigned& nb, unsigned& g) {
  const unsigned q3 = k - 128u, q4 = k - 192u, q7 = k - 320u;
  const unsigned g3 = ((q3 >> 3) * 8u + ((q3 >> 2) & 1u)) * 4u + (q3 & 3u), g4 = ((q4 >> 2) * 8u + 7u) * 4u + (q4 & 3u);
  nb = k < 64u ? 1u : k < 128u ? 2u : k < 192u ? 3u : k < 224u ? 4u : k < 288u ? 5u : k < 320u ? 6u : 7u + q7 % 20u;
  g = k < 64u ? k * 4u : k < 128u ? (k - 64u) * 4u + 3u : k < 192u ? g3 : k < 224u ? g4 : k < 288u ? k - 224u : k < 320u ? k - 96u : (q7 / 20u) * 32u;
  g &= 255u;
}

// halo_loads: MESHER: 410 as the mesher reads them, else that many (<= 512) at random granules, 0 = none
template <bool MESHER>
__global__ void __launch_bounds__(128, 5) k_mesh_shape_batch(const uint4* __restrict__ pool, const unsigned* __restrict__ slots /* [n][27] */,
                                                             uint4* __restrict__ mesh, unsigned nchunks, unsigned halo_loads) {
  __shared__ uint4 stage[256 + 416];
  __shared__ unsigned ssl[32];
  const unsigned t = threadIdx.x;
  for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const unsigned* sl = slots + (size_t)c * 27;
    ssl[t & 31u] = sl[(t & 31u) < 27u ? (t & 31u) : 26u];  // hop 1: the chunk's row (every thread, no condition; equal values per word)
    __syncthreads();
    uint4 own0, own1, hv[4];
    {
      const uint4* own = pool + (size_t)ssl[0] * 256;        // hop 2: own voxels and the thread's halo loads, one batch
      own0 = own[t]; own1 = own[128 + t];
    }
    if (halo_loads) {                                        // (uniform)
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        unsigned k = j * 128u + t, nb, g;
        if (k >= halo_loads) k = 0;                          // (a thread without a load: a mapped dummy)
        if (MESHER) halo_at(k, nb, g);
        else { nb = 1 + (k * 7u + c) % 26u; g = (k * 2654435761u + c * 40503u) >> 24; }
        hv[j] = pool[(size_t)ssl[nb] * 256 + g];
      }
      // (stored without a condition -- a dummy goes to the words 410 .. 415 nobody reads: a load whose only use sits under a
      // condition is sunk into it, and waited for there on its own)
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) { const unsigned k = j * 128u + t; stage[256 + (k < halo_loads ? k : 410u + (t & 3u))] = hv[j]; }
    }
    stage[t] = own0; stage[128 + t] = own1;
    __syncthreads();
    uint4* out = mesh + (size_t)ssl[0] * 1280;
    for (unsigned k = t; k < 264; k += 128) {
      uint4 a = stage[k % 256], b = stage[256 + (k % 410)];
      out[k] = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(128, 5) k_mesh_shape(const uint4* __restrict__ pool, const unsigned* __restrict__ slots /* [n][27] */,
                                                       uint4* __restrict__ mesh, unsigned nchunks, unsigned halo_loads) {
  __shared__ uint4 stage[256 + 416];
  const unsigned t = threadIdx.x;
  for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const unsigned* sl = slots + (size_t)c * 27;
    const uint4* own = pool + (size_t)sl[0] * 256;        // 4 KiB = 256 x 16 B
    stage[t] = own[t];
    stage[128 + t] = own[128 + t];
    if (halo_loads == 411u) {
      // variant: the two x-neighbours read WHOLE (2 x 256 coalesced granules: the same 64 lines, half the line requests),
      // the other 282 loads as below
      for (unsigned k = t; k < 512u; k += 128) { const unsigned nb = 1u + (k >> 8); const uint4 v = pool[(size_t)sl[nb] * 256 + (k & 255u)]; if ((k & 3u) == (nb == 1u ? 0u : 3u)) stage[256 + (k >> 2)] = v; }
      for (unsigned k = 128u + t; k < 410u; k += 128) {
        unsigned nb, g;
        if (k < 192u) { const unsigned q = k - 128u; nb = 3; g = ((q >> 3) * 8u + ((q >> 2) & 1u)) * 4u + (q & 3u); }
        else if (k < 224u) { const unsigned q = k - 192u; nb = 4; g = ((q >> 2) * 8u + 7u) * 4u + (q & 3u); }
        else if (k < 288u) { nb = 5; g = k - 224u; }
        else if (k < 320u) { nb = 6; g = 224u + (k - 288u); }
        else { const unsigned q = k - 320u; nb = 7u + q % 20u; g = ((q / 20u) * 8u) * 4u; }
        stage[256 + k] = pool[(size_t)sl[nb] * 256 + g];
      }
    } else if (halo_loads == 410u) {
      // the halo as the mesher reads it (x fastest: a 64-byte row holds the 8 voxels of one (z, y); 16-byte granule = 2 voxels):
      // +x / -x: first / last granule of all 64 rows; +y: rows (z, 0) and (z, 1); -y: rows (z, 7); +z: slices 0, 1; -z: slice 7;
      // 12 edge and 8 corner neighbours: a few granules each
      for (unsigned k = t; k < 410u; k += 128) {
        unsigned nb, g;
        if (k < 64u) { nb = 1; g = k * 4u; }                                   // +x: voxels x = 0, 1 of every row
        else if (k < 128u) { nb = 2; g = (k - 64u) * 4u + 3u; }                // -x: voxels x = 6, 7
        else if (k < 192u) { const unsigned q = k - 128u; nb = 3; g = ((q >> 3) * 8u + ((q >> 2) & 1u)) * 4u + (q & 3u); }  // +y: rows (z, 0), (z, 1)
        else if (k < 224u) { const unsigned q = k - 192u; nb = 4; g = ((q >> 2) * 8u + 7u) * 4u + (q & 3u); }               // -y: rows (z, 7)
        else if (k < 288u) { nb = 5; g = k - 224u; }                           // +z: slices z = 0, 1 (64 granules)
        else if (k < 320u) { nb = 6; g = 224u + (k - 288u); }                  // -z: slice z = 7
        else { const unsigned q = k - 320u; nb = 7u + q % 20u; g = ((q / 20u) * 8u) * 4u; }  // edges / corners: row starts
        stage[256 + k] = pool[(size_t)sl[nb] * 256 + g];
      }
    } else {
    for (unsigned k = t; k < halo_loads; k += 128) {      // pairs of voxels at RANDOM granules of the neighbours
      const unsigned nb = 1 + (k * 7u + c) % 26u;
      const unsigned row = (k * 2654435761u + c * 40503u) >> 24;  // 0..255: a 16-byte granule of the neighbour's 4 KiB
      stage[256 + k] = pool[(size_t)sl[nb] * 256 + row];
    }
    }
    __syncthreads();
    // "mesh": 4.2 KB out = 264 x 16 B, made of what was staged (so nothing can be dropped)
    uint4* out = mesh + (size_t)sl[0] * 1280;             // 20 KiB per pool slot
    for (unsigned k = t; k < 264; k += 128) {
      uint4 a = stage[k % 256], b = stage[256 + (k % 410)];
      out[k] = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
    }
    __syncthreads();
  }
}

int main() {
  const unsigned pool = 1u << 18;                          // 1 GiB of voxel chunks, 5 GiB of mesh blocks
  uint4 *P, *M; unsigned* S;
  CK(hipMalloc(&P, (size_t)pool * 4096)); CK(hipMalloc(&M, (size_t)pool * 20480)); CK(hipMemset(P, 1, (size_t)pool * 4096));
  hipDeviceProp_t pr; CK(hipGetDeviceProperties(&pr, 0));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float pair = 1e9f;  // an (almost) empty launch between the same two events
  {
    unsigned* S0; CK(hipMalloc(&S0, 4 * 27));
    for (int rep = 0; rep < 8; ++rep) {
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(k_mesh_shape, dim3(1), dim3(128), 0, 0, P, S0, M, 0u, 0u);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep && ms < pair) pair = ms;
    }
    printf("an empty launch between the two events: %.1f us\n", pair * 1e3);
  }
  for (unsigned n : {2929u, 11200u}) {                     // a room frame's survivors; the hall's
    std::vector<unsigned> h((size_t)n * 27 * 8);
    // neighbours of a chunk sit at unrelated pool slots (the pool is filled in visiting order), every set of chunks is new
    for (size_t i = 0; i < h.size(); ++i) h[i] = (unsigned)(((unsigned long long)(i + 12345) * 2654435761ull) % pool);
    CK(hipMalloc(&S, 4 * h.size())); CK(hipMemcpy(S, h.data(), 4 * h.size(), hipMemcpyHostToDevice));
    for (unsigned form : {0u, 1u})
    for (unsigned halo : {410u, 411u, 409u, 0u}) {  // the mesher's halo; as many loads at random granules; none
      if (form && halo == 411u) continue;            // (the whole-neighbour variant exists in the round-4 form only)
      const int grid = n < 4096u ? (int)n : 4096;
      float best = 1e9f;
      for (int rep = 0; rep < 8; ++rep) {
        CK(hipEventRecord(e0));
        if (form && halo == 410u) hipLaunchKernelGGL(k_mesh_shape_batch<true>, dim3(grid), dim3(128), 0, 0, P, S + (size_t)(rep % 8) * n * 27, M, n, halo);
        else if (form) hipLaunchKernelGGL(k_mesh_shape_batch<false>, dim3(grid), dim3(128), 0, 0, P, S + (size_t)(rep % 8) * n * 27, M, n, halo);
        else hipLaunchKernelGGL(k_mesh_shape, dim3(grid), dim3(128), 0, 0, P, S + (size_t)(rep % 8) * n * 27, M, n, halo);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep && ms < best) best = ms;
      }
      const double bytes = (double)n * (4096.0 + halo * 16.0 + 264 * 16.0);
      printf("%s %5u chunks, %3u halo loads each%s: %6.1f us, %5.2f TB/s of requested bytes (%.1f MB)\n", form ? "[batch form]  " : "[round-4 form]", n, halo, halo == 410u ? " (faces / edges as the mesher reads them)" : halo == 411u ? " (the same, x-neighbours read whole)" : halo ? " (random granules)" : "", best * 1e3, bytes / (best * 1e-3) / 1e12, bytes / 1e6);
      printf("        without the launch: %6.1f us\n", (best - pair) * 1e3);
    }
    CK(hipFree(S));
  }
  return 0;
}
