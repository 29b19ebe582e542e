// ka_math_probe.hip -- host entry points around the UNMODIFIED inline device helpers of tf_devfn.h / tf_voxel_math.h, for
// tests/test_gpu_ka_math.py.  Each entry takes host arrays, launches a one-line kernel around the helper and copies the
// results back.  Built with the library's flags (-O3 -ffp-contract=off, gfx950): tests/hip/Makefile.
// Every entry returns 0, or the hipError_t that stopped it.
#include "../../texturefusion_amd/csrc/tf_voxel_math.h"

#include <vector>

using namespace tf;

namespace {

// device copies of host arrays; freed when the entry returns
struct Bufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  template <class T>
  T* in(const T* h, size_t n) {
    T* d = out<T>(n);
    if (d && err == hipSuccess) err = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t n) {
    void* d = nullptr;
    if (err == hipSuccess) err = hipMalloc(&d, (n ? n : 1) * sizeof(T));
    if (d) p.push_back(d);
    return static_cast<T*>(d);
  }
  template <class T>
  void back(T* h, const T* d, size_t n) {
    if (err == hipSuccess) err = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
  }
  void ran() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  ~Bufs() {
    for (void* d : p) hipFree(d);
  }
};

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

__global__ void k_div2(int64_t n, const float* a0, const float* a1, const float* d, float* q0, float* q1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const f32x2 q = div2_by((f32x2){a0[i], a1[i]}, recip_refined(d[i]));
  q0[i] = q.x;
  q1[i] = q.y;
}
__global__ void k_cvt_sat(int64_t n, const float* x, int* r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) r[i] = cvt_sat_rne(x[i]);
}
__global__ void k_cvt_hw(int64_t n, const float* x, int* r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) r[i] = cvt_rne_hw(x[i]);
}
__global__ void k_truncation(int64_t n, Integ ig, const float* z, float* r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) r[i] = truncation(ig, z[i]);
}
__global__ void k_chunk_pre(int64_t n, const int* ids, Pose P, Integ ig, float res, float resDiag, float* out8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ChunkPre r = chunk_pre(make_int4(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2], 0), P.p, ig, res, resDiag);
  out8[8 * i + 0] = r.a.x; out8[8 * i + 1] = r.a.y; out8[8 * i + 2] = r.a.z; out8[8 * i + 3] = r.a.w;
  out8[8 * i + 4] = r.b.x; out8[8 * i + 5] = r.b.y; out8[8 * i + 6] = r.b.z; out8[8 * i + 7] = r.b.w;
}
__global__ void k_centroids(Pose P, float res, float* cen) { centroid_table(P.p, res, cen); }  // one workgroup of 256
__global__ void k_keys(int64_t n, const float* f, uint32_t* key, float* back) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = f2key(f[i]);
  back[i] = key2f(key[i]);
}
__global__ void k_ids(int64_t n, const int* xyz, unsigned long long* key, int* back, uint32_t* hash) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = pack_id(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  const int4 r = unpack_id(key[i]);
  back[3 * i] = r.x; back[3 * i + 1] = r.y; back[3 * i + 2] = r.z;
  hash[i] = hash_key(key[i]);
}

}  // namespace

extern "C" {

// (q0, q1)[i] = div2_by({a0[i], a1[i]}, recip_refined(d[i]))
int ka_div2(int64_t n, const float* a0, const float* a1, const float* d, float* q0, float* q1) {
  if (n <= 0) return 0;
  Bufs b;
  const float *da0 = b.in(a0, n), *da1 = b.in(a1, n), *dd = b.in(d, n);
  float *dq0 = b.out<float>(n), *dq1 = b.out<float>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_div2, grid_for(n), dim3(256), 0, 0, n, da0, da1, dd, dq0, dq1);
  b.ran();
  b.back(q0, dq0, n);
  b.back(q1, dq1, n);
  return (int)b.err;
}

int ka_cvt_sat_rne(int64_t n, const float* x, int* r) {
  if (n <= 0) return 0;
  Bufs b;
  const float* dx = b.in(x, n);
  int* dr = b.out<int>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_cvt_sat, grid_for(n), dim3(256), 0, 0, n, dx, dr);
  b.ran();
  b.back(r, dr, n);
  return (int)b.err;
}

int ka_cvt_rne_hw(int64_t n, const float* x, int* r) {
  if (n <= 0) return 0;
  Bufs b;
  const float* dx = b.in(x, n);
  int* dr = b.out<int>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_cvt_hw, grid_for(n), dim3(256), 0, 0, n, dx, dr);
  b.ran();
  b.back(r, dr, n);
  return (int)b.err;
}

// ig5 = {quad, lin, cons, scale, weight}
int ka_truncation(int64_t n, const float* ig5, const float* z, float* r) {
  if (n <= 0) return 0;
  Bufs b;
  const Integ ig = {ig5[0], ig5[1], ig5[2], ig5[3], ig5[4]};
  const float* dz = b.in(z, n);
  float* dr = b.out<float>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_truncation, grid_for(n), dim3(256), 0, 0, n, ig, dz, dr);
  b.ran();
  b.back(r, dr, n);
  return (int)b.err;
}

// out8[i] = {o.x, o.y, o.z, truncation, weight, upper, 0, 0} of chunk ids[3 i ..]
int ka_chunk_pre(int64_t n, const int* ids, const float* pose12, const float* ig5, float res, float res_diag, float* out8) {
  if (n <= 0) return 0;
  Bufs b;
  const Integ ig = {ig5[0], ig5[1], ig5[2], ig5[3], ig5[4]};
  Pose P;
  for (int q = 0; q < 12; ++q) P.p[q] = pose12[q];
  const int* di = b.in(ids, 3 * n);
  float* dr = b.out<float>(8 * n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_chunk_pre, grid_for(n), dim3(256), 0, 0, n, di, P, ig, res, res_diag, dr);
  b.ran();
  b.back(out8, dr, 8 * n);
  return (int)b.err;
}

// cen[3][512]
int ka_centroid_table(const float* pose12, float res, float* cen) {
  Bufs b;
  Pose P;
  for (int q = 0; q < 12; ++q) P.p[q] = pose12[q];
  float* dr = b.out<float>(3 * kChunkVoxels);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_centroids, dim3(1), dim3(256), 0, 0, P, res, dr);
  b.ran();
  b.back(cen, dr, 3 * kChunkVoxels);
  return (int)b.err;
}

int ka_float_keys(int64_t n, const float* f, uint32_t* key, float* back) {
  if (n <= 0) return 0;
  Bufs b;
  const float* df = b.in(f, n);
  uint32_t* dk = b.out<uint32_t>(n);
  float* db = b.out<float>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_keys, grid_for(n), dim3(256), 0, 0, n, df, dk, db);
  b.ran();
  b.back(key, dk, n);
  b.back(back, db, n);
  return (int)b.err;
}

int ka_chunk_ids(int64_t n, const int* xyz, unsigned long long* key, int* back, uint32_t* hash) {
  if (n <= 0) return 0;
  Bufs b;
  const int* dx = b.in(xyz, 3 * n);
  unsigned long long* dk = b.out<unsigned long long>(n);
  int* db = b.out<int>(3 * n);
  uint32_t* dh = b.out<uint32_t>(n);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_ids, grid_for(n), dim3(256), 0, 0, n, dx, dk, db, dh);
  b.ran();
  b.back(key, dk, n);
  b.back(back, db, 3 * n);
  b.back(hash, dh, n);
  return (int)b.err;
}

}  // extern "C"
