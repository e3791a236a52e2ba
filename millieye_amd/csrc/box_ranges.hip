// Radar range and radial speed for the detections of S independent streams: what millieye_amd/detection_range.py:range_detections
// does per stream on the host, behind me_stream_tail_f32 (csrc/nms.hip) and read straight from its output buffer, with the
// kept radar points of me_radar_proposals_f64 (csrc/radar.hip) where that chain left them.
//   box_ranges_kernel   grid (stream, chunk): validate the tail's words -> stage the stream's points in LDS -> one wave per
//                       detection row: inside test -> compaction in cloud order -> rank counting by (range, cloud index) ->
//                       c_j of every ordered point -> first j with c_j >= min_points by ballot -> the two left-to-right sums
//                       by one lane -> one row of four doubles.
// A wave keeps its own scratch in LDS and only synchronises with itself once the points are staged; the chunks of a stream
// stride over its rows, so no stream has a capacity on detections.  Every block finds the first table row of its stream by a
// parallel sum over the tail's row counts, as box_tracks_kernel does.
#include <stddef.h>

#include "common.h"

// every float64 operation is rounded on its own, like the host code's: no fused multiply-add contraction
#pragma clang fp contract(off)

namespace {

constexpr int MAXP = ME_RANGES_MAX_POINTS;
constexpr int ROWC = ME_RANGES_ROW_COLS;
constexpr int NCNT = ME_RANGES_COUNT_COLS;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PER_LANE = MAXP / 64;   // points (then ordered points) a lane owns
constexpr int MAX_CHUNKS = 64;
static_assert(MAXP % 64 == 0 && MAXP <= 65535, "whole waves of points, indices in 16 bits");
static_assert(MAXP == ME_RADAR_MAX_POINTS && NCNT == ME_RADAR_COUNT_COLS, "the radar chain's buffers");

struct WaveScratch {
  double cr[MAXP];           // ranges of the inside points, in cloud order
  double sr[MAXP], sv[MAXP]; // ranges and velocities of the inside points, ordered by (range, cloud index)
  unsigned short ci[MAXP];   // cloud index of the inside points, in cloud order
};

// LDS traffic between the lanes of one wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

__global__ __launch_bounds__(THREADS) void box_ranges_kernel(me_box_ranges_desc d) {
  __shared__ double s_pts[4][MAXP];   // u, v, range, velocity of the stream's kept points
  __shared__ WaveScratch s_wave[WAVES];
  __shared__ long long s_before[THREADS], s_total[THREADS];

  const int s = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = d.streams;
  const int32_t* hd = reinterpret_cast<const int32_t*>(d.tail_out);
  const int head = (1 + 2 * S + 3) & ~3;
  const float* table = reinterpret_cast<const float*>(hd + head);

  // ---- the tail's words: every stream's rows and kept rows; this stream's rows start behind the rows of the streams before it
  long long before = 0, total = 0;
  int bad = 0;
  for (int i = tid; i < S; i += THREADS) {
    const int rows = hd[1 + i], kept = hd[1 + S + i];
    if (rows < 0 || rows > d.m || kept < 0 || kept > rows) bad = 1;
    else {
      total += rows;
      if (i < s) before += rows;
    }
  }
  s_before[tid] = before;
  s_total[tid] = total;
  __syncthreads();
  for (int step = THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      s_before[tid] += s_before[tid + step];
      s_total[tid] += s_total[tid + step];
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  const int p = d.radar_counts[NCNT * s + ME_RANGES_POINTS_COL];
  int status = ME_RANGES_OK;
  if (hd[0] != 0 || bad || s_total[0] > d.m) status = ME_RANGES_E_INPUT;
  else if (p < 0 || p > MAXP) status = ME_RANGES_E_POINTS;
  if (chunk == 0 && tid == 0) d.status[s] = status;
  if (status != ME_RANGES_OK) return;   // uniform; no row is written
  const int row0 = (int)s_before[0];    // row0 + kept <= total <= m
  const int kept = hd[1 + S + s];
  if (chunk * WAVES >= kept) return;    // uniform

  // ---- the stream's points, column by column ---------------------------------------------------------------------------------
  const double* cloud = d.cloud_slots + (size_t)s * MAXP * 4;
  for (int e = tid; e < p * 4; e += THREADS) s_pts[e & 3][e >> 2] = cloud[e];
  __syncthreads();

  WaveScratch& w = s_wave[wave];
  const int stride = (int)gridDim.y * WAVES;
  for (int r = chunk * WAVES + wave; r < kept; r += stride) {
    const float* q = table + (size_t)(row0 + r) * 7;
    const double x1 = (double)q[0], y1 = (double)q[1], x2 = (double)q[2], y2 = (double)q[3];
    const double cx = (x1 + x2) * 0.5, cy = (y1 + y2) * 0.5;
    const double hw = ((x2 - x1) * 0.5) * d.shrink, hh = ((y2 - y1) * 0.5) * d.shrink;

    // ---- the inside points, compacted in cloud order (a NaN in the box: every comparison is false) ------------------------
    int n = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const int i = k * 64 + lane;
      bool in = false;
      if (i < p) in = fabs(s_pts[0][i] - cx) <= hw && fabs(s_pts[1][i] - cy) <= hh;
      const unsigned long long b = __ballot(in);
      if (in) {
        const int pos = n + __popcll(b & ((1ull << lane) - 1ull));
        w.cr[pos] = s_pts[2][i];
        w.ci[pos] = (unsigned short)i;
      }
      n += __popcll(b);
    }
    wave_sync();

    // ---- rank of every inside point by (range, cloud index); the compacted position grows with the cloud index --------------
    double re[PER_LANE], ve[PER_LANE];
    int rank[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const int e = k * 64 + lane;
      re[k] = e < n ? w.cr[e] : 0.0;
      ve[k] = e < n ? s_pts[3][w.ci[e] & (MAXP - 1)] : 0.0;
      rank[k] = 0;
    }
    for (int j = 0; j < n; ++j) {
      const double rj = w.cr[j];
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) rank[k] += (rj < re[k] || (rj == re[k] && j < k * 64 + lane)) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k)
      if (k * 64 + lane < n) {   // (rank < n: at most n - 1 points come before one)
        w.sr[rank[k]] = re[k];
        w.sv[rank[k]] = ve[k];
      }
    wave_sync();

    // ---- c_j = the ordered points i >= j with r_i <= r_j + gate, for the lane's j ------------------------------------------------
    double lim[PER_LANE];
    int cnt[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const int j = k * 64 + lane;
      lim[k] = j < n ? w.sr[j] + d.gate : 0.0;
      cnt[k] = 0;
    }
    for (int i = 0; i < n; ++i) {
      const double ri = w.sr[i];
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) cnt[k] += (i >= k * 64 + lane && ri <= lim[k]) ? 1 : 0;
    }

    // ---- the first j with c_j >= min_points ------------------------------------------------------------------------------------
    int first = -1, c = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const unsigned long long b = __ballot(k * 64 + lane < n && cnt[k] >= d.min_points);
      const int l = b ? __ffsll((long long)b) - 1 : 0;
      const int cl = __shfl(cnt[k], l, 64);
      if (first < 0 && b) {
        first = k * 64 + l;
        c = cl;
      }
    }

    // ---- the group's sums, left to right (first + c <= n: c_j counts points from j on) -----------------------------------------
    if (lane == 0) {
      double* o = d.ranges + (size_t)(row0 + r) * ROWC;
      if (first >= 0) {
        double sum_r = w.sr[first], sum_v = w.sv[first];
        for (int t = 1; t < c; ++t) {
          sum_r = sum_r + w.sr[first + t];
          sum_v = sum_v + w.sv[first + t];
        }
        o[0] = sum_r / (double)c;
        o[1] = sum_v / (double)c;
      } else {
        o[0] = __builtin_nan("");
        o[1] = __builtin_nan("");
      }
      o[2] = (double)c;
      o[3] = (double)n;
    }
    wave_sync();
  }
}

}  // namespace

extern "C" {

int32_t me_box_ranges_capacity(int32_t which) {
  switch (which) {
    case 0: return MAXP;
    case 1: return ROWC;
    case 2: return NCNT;
    case 3: return ME_RANGES_POINTS_COL;
    default: return -1;
  }
}

int me_box_ranges_f64(const me_box_ranges_desc* d, void* stream) {
  ME_REQUIRE(d, ME_E_NULLPTR, "me_box_ranges_f64: null descriptor");
  ME_REQUIRE(d->tail_out && d->cloud_slots && d->radar_counts && d->status && (d->ranges || d->m == 0), ME_E_NULLPTR,
             "me_box_ranges_f64: null pointer");
  ME_REQUIRE(d->streams > 0 && d->streams <= 65535 && d->m >= 0 && d->m <= 32768, ME_E_BADARG,
             "me_box_ranges_f64: %d streams, m = %d", d->streams, d->m);
  ME_REQUIRE(d->shrink == d->shrink && d->gate == d->gate && d->min_points >= 1, ME_E_BADARG,
             "me_box_ranges_f64: bad ranging parameters");
  ME_REQUIRE(me::aligned16(d->tail_out) && me::aligned16(d->cloud_slots) && me::aligned16(d->ranges), ME_E_ALIGN,
             "me_box_ranges_f64: tail_out / cloud_slots / ranges not 16-byte aligned");
  // chunks per stream: about two waves per detection row of an average stream; a stream with more rows strides over them
  long long chunks = (2LL * d->m + (long long)WAVES * d->streams - 1) / ((long long)WAVES * d->streams);
  chunks = chunks < 1 ? 1 : chunks > MAX_CHUNKS ? MAX_CHUNKS : chunks;
  hipLaunchKernelGGL(box_ranges_kernel, dim3(d->streams, (unsigned)chunks), dim3(THREADS), 0, (hipStream_t)stream, *d);
  return me::check_launch("box_ranges_kernel");
}

}  // extern "C"
