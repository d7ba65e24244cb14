// ransac_batch.h - what the RANSACs of dynoflow.hip share.  Included before the homography section:
//   ransac_sample<K>   the counter-based index sampler of every RANSAC here (homography, fundamental, PnP, point cloud, relative pose;
//                      oracle/ransac_oracle.py:sample).  Integer only.
//   ransac_bearing / ransac_cross / ransac_compose   the small fp64 helpers of the three batched motion-solver RANSACs.
//   RansacBatchDev     the common head of their per-call device structs (PnpBatchDev, PcBatchDev, RpBatchDev extend it).
//   k_ransac_score<P>  one wavefront per (problem, hypothesis), four per workgroup: the model goes through LDS and all 64 lanes test the
//                      problem's correspondences, counted with popcount(ballot) (the count does not depend on any order).
//   k_ransac_select<P> one workgroup per problem: most inliers, ties to the lowest index (a max over fixed keys, no atomics), the winner's
//                      mask recomputed with the same arithmetic, model / second output / count / index written out.
// P names a problem (PnpRansac, PcRansac, RpRansac, next to their solvers): P::Batch is its device struct, P(B, o) holds the pointers to
// the correspondences of the problem that starts at o, p.inlier(B, T, i) tests correspondence i of it against the model T (12 doubles,
// R row-major | t), and P::finish(B, prob, T, have) writes the problem's second output (run by thread 0 of k_ransac_select).
// fp64 with contraction off: the oracles under tests/ repeat every operation one rounding at a time.
#pragma once

__host__ __device__ inline uint64_t rh_splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr int RH_MAX_ATTEMPTS = 16;
constexpr int RANSAC_WAVES = 4;         // wavefronts (hypotheses) per workgroup of k_ransac_score and k_pnp_hyp

// K distinct indices in [0, n) for hypothesis h: slot j, attempt t draw from one counter; false: RH_MAX_ATTEMPTS duplicates in one slot
template <int K>
__device__ inline bool ransac_sample(int h, int n, int* idx) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    int t = 0;
    for (;;) {
      const int c = (int)(rh_splitmix64((uint64_t)h * 1315423911ull + (uint64_t)j * 2654435761ull + (uint64_t)t * 97ull) % (uint64_t)n);
      bool dup = false;
#pragma unroll
      for (int q = 0; q < j; ++q) dup = dup || idx[q] == c;
      if (!dup) { idx[j] = c; break; }
      if (++t >= RH_MAX_ATTEMPTS) return false;
    }
  }
  return true;
}

struct RansacCam { double fx, fy, skew, u0, v0; };

// the unit bearing of pixel (u, v)
#pragma clang fp contract(off)
__device__ inline void ransac_bearing(const RansacCam& C, double u, double v, double* f) {
  const double y = (v - C.v0) / C.fy;
  const double x = (u - C.u0 - C.skew * y) / C.fx;
  const double n = sqrt(x * x + y * y + 1.0);
  f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}
#pragma clang fp contract(off)
__device__ inline void ransac_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// left . T, or left itself where there is no model
#pragma clang fp contract(off)
__device__ inline void ransac_compose(const double* L, const double* T, bool have, double* out) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out[3 * i + j] = have ? (L[3 * i] * T[j] + L[3 * i + 1] * T[3 + j]) + L[3 * i + 2] * T[6 + j] : L[3 * i + j];
    out[9 + i] = have ? ((L[3 * i] * T[9] + L[3 * i + 1] * T[10]) + L[3 * i + 2] * T[11]) + L[9 + i] : L[9 + i];
  }
}

struct RansacBatchDev {
  int n_problems, n_hyp;
  const int32_t* offset;
  double threshold;
  int32_t* score;                       // scratch [n_problems * n_hyp]; -1: no model
  double* hyp_T;                        // scratch [n_problems * n_hyp * 12]
  double* T_out;
  int32_t *n_inliers, *best;
  uint8_t* inlier;
};

// the inliers of the model T among the n correspondences of p, counted by one whole wavefront
#pragma clang fp contract(off)
template <class P>
__device__ inline int ransac_count(const typename P::Batch& B, const P& p, const double* T, int n, int lane) {
  int cnt = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool in = i < n && p.inlier(B, T, i);
    cnt += __popcll(__ballot(in));
  }
  return cnt;
}

#pragma clang fp contract(off)
template <class P>
__global__ __launch_bounds__(64 * RANSAC_WAVES) void k_ransac_score(typename P::Batch B) {
  __shared__ double s_T[RANSAC_WAVES][12];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t g = (size_t)blockIdx.x * RANSAC_WAVES + w, total = (size_t)B.n_problems * B.n_hyp;
  const bool live = g < total;
  const int prob = live ? (int)(g / B.n_hyp) : 0;
  const int o = B.offset[prob], n = live ? B.offset[prob + 1] - o : 0;
  const P p(B, o);
  const bool ok = live && B.score[g] >= 0;          // uniform over the wavefront
  if (lane < 12) s_T[w][lane] = live ? B.hyp_T[12 * g + lane] : 0.0;
  __syncthreads();
  const int cnt = ok ? ransac_count(B, p, s_T[w], n, lane) : 0;
  if (live && lane == 0) B.score[g] = cnt;
}

#pragma clang fp contract(off)
template <class P>
__global__ __launch_bounds__(256) void k_ransac_select(typename P::Batch B) {
  __shared__ unsigned long long s_key[4];
  __shared__ double s_T[12];
  __shared__ int s_cnt[4];
  const int prob = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int o = B.offset[prob], n = B.offset[prob + 1] - o;
  const P p(B, o);
  const int32_t* score = B.score + (size_t)prob * B.n_hyp;
  // most inliers, ties to the lowest index: the maximum of (score << 32 | ~h) over the hypotheses with score > 0 (order-free)
  unsigned long long key = 0ull;
  for (int h = tid; h < B.n_hyp; h += 256) {
    const unsigned long long c = ((unsigned long long)(unsigned)score[h] << 32) | (unsigned)(~h);
    if (score[h] > 0 && c > key) key = c;
  }
  for (int m = 32; m > 0; m >>= 1) { const unsigned long long v = __shfl_xor(key, m, 64); if (v > key) key = v; }
  if (lane == 0) s_key[w] = key;
  __syncthreads();
  key = s_key[0];
  for (int k = 1; k < 4; ++k) if (s_key[k] > key) key = s_key[k];
  const int best = key ? (int)~(unsigned)(key & 0xFFFFFFFFull) : -1;
  if (tid < 12) s_T[tid] = best >= 0 ? B.hyp_T[12 * ((size_t)prob * B.n_hyp + best) + tid] : (tid == 0 || tid == 4 || tid == 8 ? 1.0 : 0.0);
  __syncthreads();
  int cnt = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const bool in = best >= 0 && i < n && p.inlier(B, s_T, i);
    if (i < n) B.inlier[o + i] = in ? 1 : 0;
    cnt += __popcll(__ballot(in));
  }
  if (lane == 0) s_cnt[w] = cnt;
  __syncthreads();
  if (tid == 0) {
    B.n_inliers[prob] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    B.best[prob] = best;
    for (int q = 0; q < 12; ++q) B.T_out[12 * (size_t)prob + q] = s_T[q];
    P::finish(B, prob, s_T, best >= 0);
  }
}
