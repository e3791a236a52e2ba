// Radar proposal chain of the live demos for S independent streams: what
// millieye_amd/radar_proposals.py:RadarProposalGenerator.__call__ does per stream on the host (module3_our_dataset/run_mp.py:
// 65-135 with data_collection/utils/{utils,tracking}.py), one workgroup per stream, tracker state in device memory.
//   radar_chain_kernel   gather / project / filter -> cloud -> DBSCAN (min_samples 2 = connected components) -> cluster records
//                        -> association cost + exact assignment -> Kalman predict / new tracks / Joseph update -> age filter
//                        -> confirmed tracks -> pixel proposals -> normalised network boxes.  Everything per stream goes to
//                        that stream's slots; a stream over a capacity sets its status and touches no state.
//   radar_pack_kernel    slots -> the packed [total,5] boxes of Network.forward and the packed (points, offsets) of
//                        me_radar_heatmap_f32.
//   radar_boxes_letterbox_kernel / radar_boxes_pack_kernel
//                        me_radar_boxes_letterbox_f32: the network boxes again, from the pixel proposals on the device, for a
//                        rectangular canvas (letterbox.h: the padding and the divisor per axis).
//   frame_means_kernel   one mean per frame (the auto mode's img.mean()).
// Nothing here is throughput-bound (the demos have about 25 points, 3 clusters, 4 tracks per stream; tests/test_gpu_radar_chain.py
// runs it at the capacities, 256 / 32 / 32); the point is that S streams cost two launches and no host loop.
#include <stddef.h>

#include "common.h"
#include "letterbox.h"

// the host code's float64 / float32 operations are rounded one by one: no fused multiply-add contraction
#pragma clang fp contract(off)

namespace {

constexpr int MAXP = ME_RADAR_MAX_POINTS;
constexpr int MAXC = ME_RADAR_MAX_CLUSTERS;
constexpr int MAXT = ME_RADAR_MAX_TRACKS;
constexpr int NCNT = ME_RADAR_COUNT_COLS;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
static_assert(MAXP == THREADS, "one thread per kept point");
static_assert(MAXC <= 32 && MAXT <= 32, "the assignment arrays are sized for 32 x 32");

struct ClusterRec {   // CLUSTER_DTYPE (run_mp.py:285-286), 32 bytes
  uint32_t num_points;
  float center[3];
  float size[3];
  float avgV;
};
static_assert(sizeof(ClusterRec) == 32, "cluster record layout");

struct Track {        // one KalmanClusterTracker: 96 eight-byte words
  double x[9];
  double P[81];
  ClusterRec rec;
  int32_t time_since_update, hit_streak, prev_hit_streak, pad;
};
constexpr int TRACK_WORDS = sizeof(Track) / 8;
static_assert(sizeof(Track) == 768, "track layout");

struct StreamState {  // one Tracker
  int32_t frame_count, n_tracks, pad[14];
  Track tracks[MAXT];
};

__host__ __device__ constexpr int sel(int c) { return c < 3 ? c : c + 2; }               // H: measurement c reads state sel(c)
__host__ __device__ constexpr int selinv(int j) { return j < 3 ? j : (j < 5 ? -1 : j - 2); }

// projection_xyr_to_uv (utils.py:81-101), operation for operation - except rr ** 3, which numpy takes from the C library's pow
// and this takes from the device's: the two are not guaranteed to round alike where k3 != 0.  One ulp of u or v matters only at an
// integer boundary (the truncation); the proposals are compared in float64 under a measured bar.
__device__ inline void project(double px, double py, double pr, const double* cal, double& u, double& v) {
  const double fx = cal[0], cx = cal[1], fy = cal[2], cy = cal[3], k1 = cal[4], k2 = cal[5], t1 = cal[6], t2 = cal[7],
               k3 = cal[8], tx = cal[9], ty = cal[10], tz = cal[11];
  const double depth = pr + tz;
  const double x = (px + tx) / depth, y = (py + ty) / depth;
  const double xx = x * x, yy = y * y;
  const double rr = xx + yy;
  const double radial = 1.0 + k1 * rr + k2 * (rr * rr) + k3 * pow(rr, 3.0);
  const double xd = x * radial + 2.0 * t1 * x * y + t2 * (rr + 2.0 * xx);
  const double yd = y * radial + 2.0 * t2 * x * y + t1 * (rr + 2.0 * yy);
  u = xd * fx + cx;
  v = yd * fy + cy;
}

// exclusive rank of the threads with `flag` in thread order; `total` = their number.  Called by the whole workgroup.
__device__ inline int block_rank(bool flag, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int pre = __popcll(bal & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int off = 0;
  total = 0;
  for (int w = 0; w < WAVES; ++w) {
    const int c = s_wave[w];
    if (w < wave) off += c;
    total += c;
  }
  return off + pre;
}

// numpy's pairwise sum of a 1-D float64 reduction (np.mean of the strided velocity column): blocks of at most 128 elements
// summed in eight interleaved accumulators, halves split at a multiple of eight.  a[i * stride].
__device__ double pairwise_leaf(const double* a, int n, int stride) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i * stride];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * stride];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i * stride];
  return res;
}
__device__ double pairwise_sum(const double* a, int n, int stride) {   // n <= 512: two levels of halving reach the leaves
  if (n <= 128) return pairwise_leaf(a, n, stride);
  int n2 = n / 2;
  n2 -= n2 % 8;
  double half[2];
  for (int h = 0; h < 2; ++h) {
    const double* b = h ? a + n2 * stride : a;
    const int m = h ? n - n2 : n2;
    if (m <= 128) {
      half[h] = pairwise_leaf(b, m, stride);
    } else {
      int m2 = m / 2;
      m2 -= m2 % 8;
      half[h] = pairwise_leaf(b, m2, stride) + pairwise_leaf(b + m2 * stride, m - m2, stride);
    }
  }
  return half[0] + half[1];
}

// scipy.optimize.linear_sum_assignment (rectangular_lsap.cpp: shortest augmenting paths, Crouse 2016) on cost[nr * nc],
// nr <= nc; col4row[i] = the column of row i.  One lane.
struct Lsap {
  double u[32], v[32], spc[32];
  int col4row[32], row4col[32], path[32], remaining[32];
  unsigned char SR[32], SC[32];
};
__device__ void lsap_solve(const double* cost, int nr, int nc, Lsap& w) {
  const double inf = __builtin_huge_val();
  for (int i = 0; i < nr; ++i) { w.u[i] = 0.0; w.col4row[i] = -1; }
  for (int j = 0; j < nc; ++j) { w.v[j] = 0.0; w.row4col[j] = -1; w.path[j] = -1; }
  for (int cur = 0; cur < nr; ++cur) {
    double min_val = 0.0;
    int i = cur, num_remaining = nc, sink = -1;
    for (int it = 0; it < nc; ++it) { w.remaining[it] = nc - it - 1; w.SC[it] = 0; w.spc[it] = inf; }
    for (int r = 0; r < nr; ++r) w.SR[r] = 0;
    while (sink == -1) {
      int index = -1;
      double lowest = inf;
      w.SR[i] = 1;
      for (int it = 0; it < num_remaining; ++it) {
        const int j = w.remaining[it];
        const double r = min_val + cost[i * nc + j] - w.u[i] - w.v[j];
        if (r < w.spc[j]) { w.path[j] = i; w.spc[j] = r; }
        if (w.spc[j] < lowest || (w.spc[j] == lowest && w.row4col[j] == -1)) { lowest = w.spc[j]; index = it; }
      }
      min_val = lowest;
      if (index < 0) return;   // infeasible: cannot happen with finite costs
      const int j = w.remaining[index];
      if (w.row4col[j] == -1) sink = j; else i = w.row4col[j];
      w.SC[j] = 1;
      w.remaining[index] = w.remaining[--num_remaining];
    }
    w.u[cur] += min_val;
    for (int r = 0; r < nr; ++r)
      if (w.SR[r] && r != cur) w.u[r] += min_val - w.spc[w.col4row[r]];
    for (int j = 0; j < nc; ++j)
      if (w.SC[j]) w.v[j] -= min_val - w.spc[j];
    int j = sink;
    while (true) {
      const int r = w.path[j];
      w.row4col[j] = r;
      const int t = w.col4row[r];
      w.col4row[r] = j;
      j = t;
      if (r == cur) break;
    }
  }
}

struct KalmanWs {   // per-wave scratch of the predict / update of one track
  double x[9], P[81], A[81], B[81], K[63], y[7];
};

__global__ __launch_bounds__(THREADS) void radar_chain_kernel(me_radar_desc d) {
  __shared__ double s_pt[MAXP][4];      // kept points: camera-frame (x, y, range, velocity)
  __shared__ double s_w[MAXP][4];       // the same scaled by dbscan_weights
  __shared__ unsigned s_adj[MAXP][MAXP / 32];
  __shared__ int s_lab[MAXP];           // smallest point index of the component
  __shared__ int s_dl[MAXP];            // DBSCAN label, -1 noise
  __shared__ int s_rank[MAXP];
  __shared__ unsigned char s_nb[MAXP];  // has a neighbour (= core point with min_samples 2)
  __shared__ ClusterRec s_cl[MAXC];
  __shared__ double s_cost[MAXT * MAXC];
  __shared__ Lsap s_lsap;
  __shared__ KalmanWs s_kw[WAVES];
  __shared__ int s_wave[WAVES];
  __shared__ int s_m_old[MAXT], s_m_new[MAXC], s_newlist[MAXC], s_dst[MAXT], s_trk[MAXT];
  __shared__ double s_prop[MAXT][4];
  __shared__ float s_box[MAXT][4];
  __shared__ unsigned char s_prop_ok[MAXT], s_box_ok[MAXT];
  __shared__ double s_meanv;
  __shared__ int s_status, s_bad, s_n_new, s_n_alive, s_n_trk;

  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* cal = d.calib + 12 * s;
  const int width = d.image_size[2 * s], height = d.image_size[2 * s + 1];
  StreamState* st = reinterpret_cast<StreamState*>(d.state) + s;
  int* cnt = d.counts + NCNT * s;
  double* cloud = d.cloud_slots + (size_t)s * MAXP * 4;
  if (tid == 0) { s_status = ME_RADAR_OK; s_bad = 0; }

  // ---- gather, project, filter; order-preserving compaction (from_3d_to_2d, fov_velocity_filter) -------------------
  const int r0 = d.offsets[s];
  int nin = d.offsets[s + 1] - r0;
  if (nin < 0) nin = 0;
  int kept = 0;
  for (int base = 0; base < nin; base += THREADS) {
    const int i = base + tid;
    bool keep = false;
    double px = 0, py = 0, pr = 0, pv = 0, ui = 0, vi = 0;
    if (i < nin) {
      const double* q = d.points + (size_t)(r0 + i) * 4;
      px = q[0]; py = -q[2]; pr = q[1]; pv = q[3];
      double u, v;
      project(px, py, pr, cal, u, v);
      pr = pr + cal[11];
      // astype(int64) truncates toward zero; values the cast cannot hold never pass the FOV test
      if (fabs(u) < 1e15 && fabs(v) < 1e15) {
        const long long ul = (long long)u, vl = (long long)v;
        ui = (double)ul; vi = (double)vl;
        keep = ul >= 0 && ul < width && vl >= 0 && vl < height && pr < d.max_depth && fabs(pv) >= d.min_velocity;
      }
    }
    int total;
    const int pos = kept + block_rank(keep, s_wave, total);
    if (keep && pos < MAXP) {
      s_pt[pos][0] = px; s_pt[pos][1] = py; s_pt[pos][2] = pr; s_pt[pos][3] = pv;
      cloud[pos * 4 + 0] = ui; cloud[pos * 4 + 1] = vi; cloud[pos * 4 + 2] = pr; cloud[pos * 4 + 3] = pv;
    }
    kept += total;
  }
  __syncthreads();
  if (kept > MAXP) {
    if (tid == 0) s_status = ME_RADAR_E_POINTS;
    kept = 0;   // the rest of the chain runs empty; the status check below returns before any state is written
  }
  const int n = kept;

  // ---- DBSCAN, min_samples = 2: connected components of `distance <= eps` on the weighted coordinates ---------------
  if (tid < n)
    for (int c = 0; c < 4; ++c) s_w[tid][c] = s_pt[tid][c] * d.weights[c];
  __syncthreads();
  {
    const double eps2 = d.eps * d.eps;
    bool nb = false;
    if (tid < n) {
      const double a0 = s_w[tid][0], a1 = s_w[tid][1], a2 = s_w[tid][2], a3 = s_w[tid][3];
      for (int wd = 0; wd < MAXP / 32; ++wd) {
        unsigned bits = 0;
        for (int b = 0; b < 32; ++b) {
          const int j = wd * 32 + b;
          if (j >= n) break;
          const double e0 = a0 - s_w[j][0], e1 = a1 - s_w[j][1], e2 = a2 - s_w[j][2], e3 = a3 - s_w[j][3];
          const double d2 = e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
          if (d2 <= eps2 && j != tid) bits |= 1u << b;
        }
        s_adj[tid][wd] = bits;
        nb = nb || bits != 0;
      }
      s_lab[tid] = tid;
      s_nb[tid] = nb;
    }
  }
  __syncthreads();
  for (int iter = 0; iter <= MAXP; ++iter) {   // label propagation to the fixed point (at most the longest chain)
    int m = MAXP;
    if (tid < n) {
      m = s_lab[tid];
      for (int wd = 0; wd < (n + 31) / 32; ++wd) {
        unsigned bits = s_adj[tid][wd];
        while (bits) {
          const int b = __ffs(bits) - 1;
          bits &= bits - 1;
          const int l = s_lab[wd * 32 + b];
          m = l < m ? l : m;
        }
      }
    }
    __syncthreads();
    int changed = 0;
    if (tid < n && m < s_lab[tid]) { s_lab[tid] = m; changed = 1; }
    if (!__syncthreads_or(changed)) break;
  }
  // clusters are numbered by their smallest point index
  int ncomp;
  {
    const bool root = tid < n && s_nb[tid] && s_lab[tid] == tid;
    const int rk = block_rank(root, s_wave, ncomp);
    if (root) s_rank[tid] = rk;
  }
  __syncthreads();
  if (tid < n) {
    const int l = s_nb[tid] ? s_rank[s_lab[tid]] : -1;
    s_dl[tid] = l;
    if (d.labels) d.labels[(size_t)s * MAXP + tid] = l;
  }
  __syncthreads();

  // ---- cluster records (radar_dbscan) and the num_pts filter -------------------------------------------------------
  if (tid == THREADS - 1) s_meanv = n > 0 ? pairwise_sum(&s_pt[0][3], n, 4) / (double)n : 0.0;  // quirk: ALL kept points
  ClusterRec rec = {};
  bool pass = false;
  if (tid < ncomp) {   // at most n / 2 <= 128 components
    double sum[3] = {0.0, 0.0, 0.0}, mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int count = 0;
    for (int i = 0; i < n; ++i) {
      if (s_dl[i] != tid) continue;
      for (int c = 0; c < 3; ++c) {
        const double val = s_pt[i][c];
        sum[c] += val;
        mn[c] = count == 0 || val < mn[c] ? val : mn[c];
        mx[c] = count == 0 || val > mx[c] ? val : mx[c];
      }
      ++count;
    }
    rec.num_points = (uint32_t)count;
    for (int c = 0; c < 3; ++c) {
      rec.center[c] = (float)(sum[c] / (double)count);
      rec.size[c] = (float)(mx[c] - mn[c]);
    }
    pass = count >= d.num_pts_filter;
  }
  int nclu;
  {
    const int pos = block_rank(pass, s_wave, nclu);   // (its barriers also publish s_meanv)
    if (pass && pos < MAXC) {
      rec.avgV = (float)s_meanv;
      s_cl[pos] = rec;
    }
  }
  __syncthreads();
  if (nclu > MAXC) {
    if (tid == 0 && s_status == ME_RADAR_OK) s_status = ME_RADAR_E_CLUSTERS;
    nclu = 0;
  }

  // ---- association (associate_clusters): float32 cost, exact assignment ----------------------------------------------
  int T = st->n_tracks;
  if (T < 0 || T > MAXT) T = 0;   // (a state that was never reset)
  for (int e = tid; e < T * nclu; e += THREADS) {
    const int i = e / nclu, j = e - i * nclu;
    const ClusterRec& o = st->tracks[i].rec;
    const ClusterRec& c = s_cl[j];
    const float ahead = o.center[2] + o.avgV / 20.f;
    const float d0 = c.center[0] - o.center[0], d1 = c.center[1] - o.center[1], d2 = c.center[2] - ahead;
    const float cost = (1.f * (d0 * d0) + 1.f * (d1 * d1)) + 10.f * (d2 * d2);
    if (!(fabsf(cost) <= 3.4028234e38f)) s_bad = 1;
    // scipy transposes a matrix with more rows than columns
    if (T <= nclu) s_cost[i * nclu + j] = (double)cost; else s_cost[j * T + i] = (double)cost;
  }
  if (tid < MAXT) s_m_old[tid] = -1;
  if (tid < MAXC) s_m_new[tid] = -1;
  __syncthreads();
  if (tid == 0) {
    if (s_bad && s_status == ME_RADAR_OK) s_status = ME_RADAR_E_COST;
    int n_new = 0;
    if (s_status == ME_RADAR_OK) {
      if (T > 0 && nclu > 0) {
        if (T <= nclu) {
          lsap_solve(s_cost, T, nclu, s_lsap);
          for (int i = 0; i < T; ++i) { const int j = s_lsap.col4row[i]; if (j >= 0) { s_m_old[i] = j; s_m_new[j] = i; } }
        } else {
          lsap_solve(s_cost, nclu, T, s_lsap);
          for (int j = 0; j < nclu; ++j) { const int i = s_lsap.col4row[j]; if (i >= 0) { s_m_old[i] = j; s_m_new[j] = i; } }
        }
      }
      for (int j = 0; j < nclu; ++j)
        if (s_m_new[j] < 0) s_newlist[n_new++] = j;
      // A complete rectangular assignment leaves max(0, nclu - T) clusters unmatched, so T + n_new = max(T, nclu) <= 32 while
      // MAXC <= MAXT: this cannot fire.  It guards the appends below against a change of the capacities.
      if (T + n_new > MAXT) s_status = ME_RADAR_E_TRACKS;
    }
    s_n_new = n_new;
  }
  __syncthreads();
  if (s_status != ME_RADAR_OK) {   // nothing of the state has been written
    if (tid < NCNT) cnt[tid] = tid == 0 ? s_status : 0;
    return;
  }
  if (d.matches && tid < MAXT) d.matches[(size_t)s * MAXT + tid] = tid < T ? s_m_old[tid] : -1;
  if (tid < nclu) reinterpret_cast<ClusterRec*>(d.clusters)[(size_t)s * MAXC + tid] = s_cl[tid];

  // ---- predict every track, update the matched ones (KalmanClusterTracker.predict / .update): one wave per track ----
  const double dt = d.dt;
  for (int base = 0; base < T; base += WAVES) {
    const int ti = base + wave;
    const bool active = ti < T;
    Track* trk = st->tracks + (active ? ti : 0);
    KalmanWs& w = s_kw[wave];
    const int mj = active ? s_m_old[ti] : -1;
    int tsu = 0, hs = 0, phs = 0;
    if (active) {
      for (int e = lane; e < 81; e += 64) w.P[e] = trk->P[e];
      if (lane < 9) w.x[lane] = trk->x[lane];
      tsu = trk->time_since_update; hs = trk->hit_streak; phs = trk->prev_hit_streak;
    }
    __syncthreads();
    // predict: x <- F x, P <- F P F' + Q with F = I + dt on (0,3), (1,4), (2,5).  The matrix-matrix products here and in the
    // update accumulate k = 0, 1, .. with one fused multiply-add per term - what the host's BLAS matrix product does (its products
    // with the exact zeros and ones of F, H and R change nothing); the matrix-vector products are left unfused.
    double xn = 0.0;
    if (active) {
      for (int e = lane; e < 81; e += 64) w.B[e] = e < 27 ? fma(dt, w.P[e + 27], w.P[e]) : w.P[e];
      if (lane < 3) xn = w.x[lane] + dt * w.x[lane + 3];
    }
    __syncthreads();
    if (active) {
      for (int e = lane; e < 81; e += 64) {
        const int i = e / 9, j = e - i * 9;
        const double q = i != j ? 0.0 : (i < 6 ? 0.03 : 0.03 * 0.05);
        w.P[e] = (j < 3 ? fma(w.B[e + 3], dt, w.B[e]) : w.B[e]) + q;
      }
      if (lane < 3) w.x[lane] = xn;
      if (tsu == d.max_age) { phs = hs; hs = 0; }
      tsu += 1;
    }
    __syncthreads();
    // update(z): y = z - H x, S = H P H' + R, K = (P H') S^-1 through the explicit inverse, as the host code forms it
    // (np.linalg.inv, then a matrix product): the rows of K that belong to the unobserved velocities are sums of large terms
    // that cancel, and a gain solved for directly rounds them differently.  Lane c eliminates S against the unit vector e_c in
    // registers (S is symmetric positive definite: no pivoting) and leaves column c of the inverse in w.B.
    if (mj >= 0) {
      const ClusterRec& c = s_cl[mj];
      if (lane < 7) {
        const double z = lane < 3 ? (double)c.center[lane] : (lane == 3 ? (double)c.avgV : (double)c.size[lane - 4]);
        w.y[lane] = z - w.x[sel(lane)];
        double a[7][7], b[7], k[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
          for (int j = 0; j < 7; ++j) a[i][j] = w.P[sel(i) * 9 + sel(j)] + (i == j ? 1.0 : 0.0);
          b[i] = i == lane ? 1.0 : 0.0;
        }
#pragma unroll
        for (int p = 0; p < 7; ++p) {
#pragma unroll
          for (int i = p + 1; i < 7; ++i) {
            const double f = a[i][p] / a[p][p];
#pragma unroll
            for (int j = p + 1; j < 7; ++j) a[i][j] -= f * a[p][j];
            b[i] -= f * b[p];
          }
        }
#pragma unroll
        for (int i = 6; i >= 0; --i) {
          double acc = b[i];
#pragma unroll
          for (int j = i + 1; j < 7; ++j) acc -= a[i][j] * k[j];
          k[i] = acc / a[i][i];
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) w.B[i * 7 + lane] = k[i];
      }
    }
    __syncthreads();
    if (mj >= 0 && lane < 63) {   // K = (P H') S^-1
      const int r = lane / 7, c = lane - r * 7;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 7; ++k) acc = fma(w.P[r * 9 + sel(k)], w.B[k * 7 + c], acc);
      w.K[lane] = acc;
    }
    __syncthreads();
    if (mj >= 0) {
      if (lane < 9) {
        double acc = 0.0;
        for (int c = 0; c < 7; ++c) acc += w.K[lane * 7 + c] * w.y[c];
        w.x[lane] = w.x[lane] + acc;
      }
      for (int e = lane; e < 81; e += 64) {   // A = I - K H
        const int i = e / 9, j = e - i * 9, c = selinv(j);
        w.A[e] = (i == j ? 1.0 : 0.0) - (c >= 0 ? w.K[i * 7 + c] : 0.0);
      }
    }
    __syncthreads();
    if (mj >= 0)
      for (int e = lane; e < 81; e += 64) {   // B = A P
        const int i = e / 9, j = e - i * 9;
        double acc = 0.0;
        for (int k = 0; k < 9; ++k) acc = fma(w.A[i * 9 + k], w.P[k * 9 + j], acc);
        w.B[e] = acc;
      }
    __syncthreads();
    double pn[2] = {0.0, 0.0};
    if (mj >= 0) {
      for (int e = lane, q = 0; e < 81; e += 64, ++q) {   // P = (A P) A' + K R K', R = I
        const int i = e / 9, j = e - i * 9;
        double acc = 0.0, kk = 0.0;
        for (int k = 0; k < 9; ++k) acc = fma(w.B[i * 9 + k], w.A[j * 9 + k], acc);
        for (int c = 0; c < 7; ++c) kk = fma(w.K[i * 7 + c], w.K[j * 7 + c], kk);
        pn[q] = acc + kk;
      }
      tsu = 0;
      hs += 1;
    }
    __syncthreads();
    if (active) {
      for (int e = lane, q = 0; e < 81; e += 64, ++q) trk->P[e] = mj >= 0 ? pn[q] : w.P[e];
      if (lane < 9) trk->x[lane] = w.x[lane];
      if (lane == 0) {   // _write_back
        for (int c = 0; c < 3; ++c) {
          trk->rec.center[c] = (float)w.x[c];
          trk->rec.size[c] = (float)w.x[6 + c];
        }
        trk->rec.avgV = (float)w.x[5];
        if (mj >= 0) trk->rec.num_points = s_cl[mj].num_points;
        trk->time_since_update = tsu; trk->hit_streak = hs; trk->prev_hit_streak = phs;
      }
    }
    __syncthreads();
  }

  // ---- new tracks from the unmatched clusters, appended in cluster order (KalmanClusterTracker.__init__) -------------
  const int n_new = s_n_new;
  for (int k = 0; k < n_new; ++k) {
    Track* trk = st->tracks + T + k;
    const ClusterRec& c = s_cl[s_newlist[k]];
    if (tid < 81) {
      const int i = tid / 9, j = tid - i * 9;
      trk->P[tid] = i != j ? 0.0 : (i < 2 ? 10.0 : (i == 2 || i == 5 ? 1.0 : 1000.0));
    }
    if (tid < 9)
      trk->x[tid] = tid < 3 ? (double)c.center[tid] : (tid == 5 ? (double)c.avgV : (tid >= 6 ? (double)c.size[tid - 6] : 0.0));
    if (tid == 0) {
      trk->rec = c;
      trk->time_since_update = 0; trk->hit_streak = 0; trk->prev_hit_streak = 0; trk->pad = 0;
    }
  }
  __syncthreads();

  // ---- age filter (order-preserving, in place), confirmation rule ---------------------------------------------------------
  const int Tn = T + n_new;
  if (tid == 0) {
    int alive = 0, ntrk = 0;
    const int frame_count = st->frame_count + 1;
    for (int k = 0; k < Tn; ++k) {
      const Track& t = st->tracks[k];
      if (t.time_since_update <= d.max_age) {
        const int best = t.hit_streak > t.prev_hit_streak ? t.hit_streak : t.prev_hit_streak;
        if (best >= d.min_hits || frame_count <= d.min_hits) s_trk[ntrk++] = alive;
        s_dst[k] = alive++;
      } else {
        s_dst[k] = -1;
      }
    }
    s_n_alive = alive; s_n_trk = ntrk;
    st->frame_count = frame_count;
    st->n_tracks = alive;
  }
  __syncthreads();
  for (int k = 0; k < Tn; ++k) {
    const int dst = s_dst[k];
    if (dst >= 0 && dst != k) {   // dst < k: never a slot a later track still has to be read from
      if (tid < TRACK_WORDS)
        reinterpret_cast<unsigned long long*>(st->tracks + dst)[tid] = reinterpret_cast<const unsigned long long*>(st->tracks + k)[tid];
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- box proposals (box_proposals) and the network's radar boxes (radar_boxes_for_network) -------------------------------
  const int ntrk = s_n_trk;
  if (tid < ntrk) {
    const ClusterRec c = st->tracks[s_trk[tid]].rec;
    reinterpret_cast<ClusterRec*>(d.tracked)[(size_t)s * MAXT + tid] = c;
    const double c0 = c.center[0], c1 = c.center[1], c2 = c.center[2];
    const double z0 = c.size[0], z1 = c.size[1], z2 = c.size[2];
    double m = z0;
    if (z1 > m) m = z1;
    if (z2 > m) m = z2;
    const bool ok = m < d.max_size;
    bool box_ok = false;
    if (ok) {
      const double h0 = z0 * 1.0 / 2.0, h1 = z1 * 1.0 / 2.0, h2 = z2 * 0.0 / 2.0;
      double u0, v0, u1, v1;
      project(c0 + h0, c1 + h1, c2 + h2, cal, u0, v0);
      project(c0 - h0, c1 - h1, c2 - h2, cal, u1, v1);
      const double x = (u0 + u1) / 2.0;
      double y = (v0 + v1) / 2.0, bw = u0 - u1, bh = v0 - v1;
      y = y + (bh / 5.0) * 0.8;
      bw = bw * 1.2;
      bh = bh * 1.4;
      const double p0 = x - bw / 2.0, p1 = y - bh / 2.0, p2 = x + bw / 2.0, p3 = y + bh / 2.0;
      s_prop[tid][0] = p0; s_prop[tid][1] = p1; s_prop[tid][2] = p2; s_prop[tid][3] = p3;
      // + pad_to_square amounts, / padded side, clamp, drop empty boxes (float32 like the torch code)
      const int fw = d.frame_size[2 * s], fh = d.frame_size[2 * s + 1];
      const int diff = fh > fw ? fh - fw : fw - fh;
      const int pad1 = diff / 2, pad2 = diff - pad1;
      const float left = fh <= fw ? 0.f : (float)pad1, right = fh <= fw ? 0.f : (float)pad2;
      const float top = fh <= fw ? (float)pad1 : 0.f, bottom = fh <= fw ? (float)pad2 : 0.f;
      const float side = (float)(fh > fw ? fh : fw);
      float b[4] = {(float)p0 + left, (float)p1 + top, (float)p2 + right, (float)p3 + bottom};
      for (int q = 0; q < 4; ++q) {
        float val = b[q] / side;
        val = val < 0.f ? 0.f : val;   // torch.clamp keeps NaN
        val = val > 1.f ? 1.f : val;
        s_box[tid][q] = val;
        b[q] = val;
      }
      box_ok = b[0] < b[2] && b[1] < b[3];
    }
    s_prop_ok[tid] = ok;
    s_box_ok[tid] = box_ok;
  }
  __syncthreads();
  if (tid == 0) {
    int np = 0, nb = 0;
    double* prop = d.proposals + (size_t)s * MAXT * 4;
    float* boxes = d.boxes + (size_t)s * MAXT * 5;   // slot region of the packed tensor's workspace twin (see the pack kernel)
    for (int k = 0; k < ntrk; ++k) {
      if (!s_prop_ok[k]) continue;
      for (int q = 0; q < 4; ++q) prop[np * 4 + q] = s_prop[k][q];
      ++np;
      if (!s_box_ok[k]) continue;
      boxes[nb * 5] = (float)s;
      for (int q = 0; q < 4; ++q) boxes[nb * 5 + 1 + q] = s_box[k][q];
      ++nb;
    }
    cnt[0] = ME_RADAR_OK; cnt[1] = n; cnt[2] = nclu; cnt[3] = ntrk; cnt[4] = nb; cnt[5] = s_n_alive;
    cnt[6] = st->frame_count; cnt[7] = np;
  }
}

// Slots -> packed.  Workgroup s moves stream s's boxes (written by the chain kernel into slot s of `box_slots`) and cloud rows
// behind those of the streams before it; workgroup 0 also writes the offsets and the totals.
__global__ __launch_bounds__(THREADS) void radar_pack_kernel(const int* __restrict__ counts, const float* __restrict__ box_slots,
                                                             const double* __restrict__ cloud_slots, int streams,
                                                             float* __restrict__ boxes, double* __restrict__ cloud,
                                                             int* __restrict__ cloud_offsets, int* __restrict__ totals) {
  __shared__ int s_sum[2][THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  int pb = 0, pp = 0;
  for (int i = tid; i < s; i += THREADS) {
    pb += counts[NCNT * i + 4];
    pp += counts[NCNT * i + 1];
  }
  s_sum[0][tid] = pb;
  s_sum[1][tid] = pp;
  __syncthreads();
  for (int step = THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      s_sum[0][tid] += s_sum[0][tid + step];
      s_sum[1][tid] += s_sum[1][tid + step];
    }
    __syncthreads();
  }
  const int box0 = s_sum[0][0], pt0 = s_sum[1][0];
  const int nb = counts[NCNT * s + 4], np = counts[NCNT * s + 1];
  for (int e = tid; e < nb * 5; e += THREADS) boxes[(size_t)box0 * 5 + e] = box_slots[(size_t)s * MAXT * 5 + e];
  for (int e = tid; e < np * 4; e += THREADS) cloud[(size_t)pt0 * 4 + e] = cloud_slots[(size_t)s * MAXP * 4 + e];
  if (tid == 0) {
    cloud_offsets[s] = pt0;
    if (s == streams - 1) {
      cloud_offsets[streams] = pt0 + np;
      totals[0] = box0 + nb;
      totals[1] = pt0 + np;
    }
  }
}

// ---- the network's radar boxes for a rectangular canvas ------------------------------------------------------------------------
// The chain kernel's last block per axis, from what the chain left on the device: pixel proposals [streams, MAXT, 4], their
// number counts[:, 7], frame_size [streams, 2] = (w, h).  The frame is letterboxed into the canvas (letterbox.h: Ph x Pw, the
// padding split per axis), so x takes + left | right and / Pw, y takes + top | bottom and / Ph - the chain's float32 operations
// in the chain's order; a = b = 1 (square canvas) gives the chain's own rows and counts.  One wave per stream writes slot s of
// `slots` and box_counts[s]; the pack kernel moves the slots stream-major to the front and writes the total.
constexpr int BOX_THREADS = 64;

__global__ __launch_bounds__(BOX_THREADS) void radar_boxes_letterbox_kernel(const double* __restrict__ proposals,
                                                                            const int* __restrict__ counts,
                                                                            const int* __restrict__ frame_size, int a, int b,
                                                                            float* __restrict__ slots,
                                                                            int* __restrict__ box_counts) {
  __shared__ float s_box[MAXT][4];
  __shared__ int s_ok[MAXT];
  const int s = blockIdx.x, tid = threadIdx.x;
  int np = counts[NCNT * s + 7];
  np = np < 0 ? 0 : (np > MAXT ? MAXT : np);
  const int fw = frame_size[2 * s], fh = frame_size[2 * s + 1];
  const bool frame_ok = fw > 0 && fh > 0 && fw <= (1 << 30) && fh <= (1 << 30);
  const LetterboxGeom geo = letterbox_geom(frame_ok ? fh : 1, frame_ok ? fw : 1, a, b);
  if (!frame_ok || !geo.ok) np = 0;   // no canvas to normalise for: no boxes
  if (tid < np) {
    const double* p = proposals + ((size_t)s * MAXT + tid) * 4;
    const float left = (float)geo.left, right = (float)(geo.Pw - fw - geo.left);
    const float top = (float)geo.top, bottom = (float)(geo.Ph - fh - geo.top);
    const float side_x = (float)geo.Pw, side_y = (float)geo.Ph;
    float v[4] = {(float)p[0] + left, (float)p[1] + top, (float)p[2] + right, (float)p[3] + bottom};
    for (int q = 0; q < 4; ++q) {
      float val = v[q] / ((q & 1) ? side_y : side_x);
      val = val < 0.f ? 0.f : val;   // torch.clamp keeps NaN
      val = val > 1.f ? 1.f : val;
      s_box[tid][q] = val;
      v[q] = val;
    }
    s_ok[tid] = v[0] < v[2] && v[1] < v[3];
  }
  __syncthreads();
  if (tid == 0) {
    int nb = 0;
    float* out = slots + (size_t)s * MAXT * 5;
    for (int k = 0; k < np; ++k) {
      if (!s_ok[k]) continue;
      out[nb * 5] = (float)s;
      for (int q = 0; q < 4; ++q) out[nb * 5 + 1 + q] = s_box[k][q];
      ++nb;
    }
    box_counts[s] = nb;
  }
}

__global__ __launch_bounds__(THREADS) void radar_boxes_pack_kernel(const float* __restrict__ slots, int streams,
                                                                   float* __restrict__ boxes, int* __restrict__ box_counts) {
  __shared__ int s_sum[THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  int pb = 0;
  for (int i = tid; i < s; i += THREADS) pb += box_counts[i];
  s_sum[tid] = pb;
  __syncthreads();
  for (int step = THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) s_sum[tid] += s_sum[tid + step];
    __syncthreads();
  }
  const int box0 = s_sum[0], nb = box_counts[s];
  for (int e = tid; e < nb * 5; e += THREADS) boxes[(size_t)box0 * 5 + e] = slots[(size_t)s * MAXT * 5 + e];
  if (tid == 0 && s == streams - 1) box_counts[streams] = box0 + nb;
}

// ---- per-frame means ---------------------------------------------------------------------------------------------------------
constexpr int MEAN_THREADS = 1024;
// modes (me_frame_modes_f32; nullptr = means only): the auto mode's rule on the mean just stored, compared in double like the
// host's ``float(mean) < dark_threshold``: 0 = fusion (dark frame), 1 = camera only.
__global__ __launch_bounds__(MEAN_THREADS) void frame_means_kernel(const float* __restrict__ imgs, long long elems,
                                                                   float* __restrict__ means, double threshold,
                                                                   int* __restrict__ modes) {
  __shared__ double s_part[MEAN_THREADS];
  const float* x = imgs + (size_t)blockIdx.x * elems;
  double acc = 0.0;
  if ((elems & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (long long i = threadIdx.x; i < elems / 4; i += MEAN_THREADS) {
      const float4 v = x4[i];
      acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
  } else {
    for (long long i = threadIdx.x; i < elems; i += MEAN_THREADS) acc += (double)x[i];
  }
  s_part[threadIdx.x] = acc;
  __syncthreads();
  for (int step = MEAN_THREADS / 2; step > 0; step >>= 1) {
    if (threadIdx.x < step) s_part[threadIdx.x] += s_part[threadIdx.x + step];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float mean = (float)(s_part[0] / (double)elems);
    means[blockIdx.x] = mean;
    if (modes) modes[blockIdx.x] = ((double)mean < threshold) ? 0 : 1;
  }
}

}  // namespace

extern "C" {

int32_t me_radar_capacity(int32_t which) {
  switch (which) {
    case 0: return MAXP;
    case 1: return MAXC;
    case 2: return MAXT;
    case 3: return NCNT;
    case 4: return (int32_t)offsetof(StreamState, tracks);
    case 5: return (int32_t)sizeof(Track);
    default: return -1;
  }
}

int64_t me_radar_tracker_state_bytes(int32_t streams) { return streams > 0 ? (int64_t)streams * (int64_t)sizeof(StreamState) : 0; }

int me_radar_tracker_reset(void* state, int32_t streams, int32_t which, void* stream) {
  ME_REQUIRE(state, ME_E_NULLPTR, "me_radar_tracker_reset: null pointer");
  ME_REQUIRE(streams > 0 && which < streams, ME_E_BADARG, "me_radar_tracker_reset: stream %d of %d", which, streams);
  StreamState* st = reinterpret_cast<StreamState*>(state);
  if (which < 0)
    ME_HIP(hipMemsetAsync(st, 0, sizeof(StreamState) * (size_t)streams, (hipStream_t)stream));
  else
    ME_HIP(hipMemsetAsync(st + which, 0, sizeof(StreamState), (hipStream_t)stream));
  return 0;
}

int me_radar_proposals_f64(const me_radar_desc* d, void* stream) {
  ME_REQUIRE(d, ME_E_NULLPTR, "me_radar_proposals_f64: null descriptor");
  if (d->streams == 0) return 0;
  ME_REQUIRE(d->points && d->offsets && d->calib && d->image_size && d->frame_size && d->state && d->cloud_slots && d->clusters &&
                 d->tracked && d->proposals && d->counts && d->boxes && d->cloud && d->cloud_offsets && d->totals,
             ME_E_NULLPTR, "me_radar_proposals_f64: null pointer");
  ME_REQUIRE(d->streams > 0 && d->streams <= 65535, ME_E_BADARG, "me_radar_proposals_f64: %d streams", d->streams);
  ME_REQUIRE(d->max_age >= 0 && d->min_hits >= 0 && d->dt > 0.0 && d->eps >= 0.0, ME_E_BADARG,
             "me_radar_proposals_f64: bad tracker / clustering parameters");
  ME_REQUIRE(me::aligned16(d->state) && me::aligned16(d->clusters) && me::aligned16(d->tracked), ME_E_ALIGN,
             "me_radar_proposals_f64: state / clusters / tracked not 16-byte aligned");
  // the chain kernel writes a stream's boxes into slot s of the box buffer's second half; the pack kernel moves them to the front
  me_radar_desc k = *d;
  float* box_slots = d->boxes + (size_t)d->streams * MAXT * 5;
  k.boxes = box_slots;
  hipLaunchKernelGGL(radar_chain_kernel, dim3(d->streams), dim3(THREADS), 0, (hipStream_t)stream, k);
  int rc = me::check_launch("radar_chain_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(radar_pack_kernel, dim3(d->streams), dim3(THREADS), 0, (hipStream_t)stream, d->counts, box_slots,
                     d->cloud_slots, d->streams, d->boxes, d->cloud, d->cloud_offsets, d->totals);
  return me::check_launch("radar_pack_kernel");
}

int me_radar_boxes_letterbox_f32(const double* proposals, const int32_t* counts, const int32_t* frame_size, int32_t streams,
                                 int32_t height, int32_t width, float* boxes, int32_t* box_counts, void* stream) {
  if (streams == 0) return 0;
  ME_REQUIRE(proposals && counts && frame_size && boxes && box_counts, ME_E_NULLPTR, "me_radar_boxes_letterbox_f32: null pointer");
  ME_REQUIRE(streams > 0 && streams <= 65535, ME_E_BADARG, "me_radar_boxes_letterbox_f32: %d streams", streams);
  ME_REQUIRE(height > 0 && width > 0 && (long long)height * width < (1ll << 30), ME_E_BADARG,
             "me_radar_boxes_letterbox_f32: bad canvas %d x %d", height, width);
  // like the chain: a stream's boxes go to slot s of the buffer's second half, the pack kernel moves them to the front
  float* slots = boxes + (size_t)streams * MAXT * 5;
  const int g = me::gcd_i32(height, width);
  hipLaunchKernelGGL(radar_boxes_letterbox_kernel, dim3(streams), dim3(BOX_THREADS), 0, (hipStream_t)stream, proposals, counts,
                     frame_size, height / g, width / g, slots, box_counts);
  int rc = me::check_launch("radar_boxes_letterbox_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(radar_boxes_pack_kernel, dim3(streams), dim3(THREADS), 0, (hipStream_t)stream, slots, streams, boxes,
                     box_counts);
  return me::check_launch("radar_boxes_pack_kernel");
}

int me_frame_means_f32(const float* imgs, int32_t n, int64_t elems_per_frame, float* means, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(imgs && means, ME_E_NULLPTR, "me_frame_means_f32: null pointer");
  ME_REQUIRE(n > 0 && elems_per_frame > 0, ME_E_BADARG, "me_frame_means_f32: bad n / elems_per_frame");
  hipLaunchKernelGGL(frame_means_kernel, dim3(n), dim3(MEAN_THREADS), 0, (hipStream_t)stream, imgs, (long long)elems_per_frame,
                     means, 0.0, (int*)nullptr);
  return me::check_launch("frame_means_kernel");
}

int me_frame_modes_f32(const float* imgs, int32_t n, int64_t elems_per_frame, double threshold, float* means, int32_t* modes,
                       void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(imgs && means && modes, ME_E_NULLPTR, "me_frame_modes_f32: null pointer");
  ME_REQUIRE(n > 0 && elems_per_frame > 0, ME_E_BADARG, "me_frame_modes_f32: bad n / elems_per_frame");
  hipLaunchKernelGGL(frame_means_kernel, dim3(n), dim3(MEAN_THREADS), 0, (hipStream_t)stream, imgs, (long long)elems_per_frame,
                     means, threshold, modes);
  return me::check_launch("frame_means_kernel");
}

}  // extern "C"
