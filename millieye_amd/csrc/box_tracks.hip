// Track ids for the detections of S independent streams: what millieye_amd/detection_tracks.py:DetectionTracker.step does per
// stream on the host (a SORT-shaped tracker, Bewley et al. 2016: constant-velocity Kalman filter per box, IoU association by
// scipy.optimize.linear_sum_assignment, births, deaths, the min_hits rule), one workgroup per stream, tracker state in device
// memory, input read straight from the output buffer of me_stream_tail_f32 (csrc/nms.hip).
//   box_tracks_kernel   validate -> predict -> IoU matrix -> exact assignment -> gate -> Joseph update / births -> deaths
//                       -> commit -> output rows.  Everything happens on an LDS copy of the stream's state; a stream with a
//                       status writes its counts and nothing else.
// The assignment restates scipy's rectangular_lsap.cpp (shortest augmenting paths, Crouse 2016) like lsap_solve of
// csrc/radar.hip, which stays the serial statement of it; here the column scan of one augmentation step runs a column per lane
// in wave 0 (at most 64 columns).  Lane `it` holds the column at position `it` of the serial code's `remaining` list, so the
// serial scan order is the lane order and the pick - the first column at the minimum, replaced by the last later column at
// the minimum that has no row - is two ballots; the swap-removal moves the last lane's column into the freed lane.
// The eight-state filter with diagonal Q, R and birth P is four independent (coordinate, velocity) filters; the kernel keeps
// the four 2 x 2 covariance blocks and runs the operations of tests/box_tracks_refs.py's decoupled filter in its order.
#include <stddef.h>

#include "common.h"

// every float64 operation is rounded on its own, like the host code's: no fused multiply-add contraction
#pragma clang fp contract(off)

namespace {

constexpr int MAXD = ME_TRACKS_MAX_DETS;
constexpr int MAXT = ME_TRACKS_MAX_TRACKS;
constexpr int ROWC = ME_TRACKS_ROW_COLS;
constexpr int NCNT = ME_TRACKS_COUNT_COLS;
constexpr int THREADS = 256;
static_assert(MAXD <= 64 && MAXT <= 64, "one column per lane of one wave");
static_assert(MAXD <= THREADS && MAXT <= THREADS, "one thread per detection / track");

struct Track {   // 224 bytes
  double x[8];       // cx, cy, w, h, vcx, vcy, vw, vh
  double P[4][4];    // per coordinate c: [[P(c,c), P(c,c+4)], [P(c+4,c), P(c+4,c+4)]] row-major
  int32_t id;
  float cls, conf;
  int32_t time_since_update, hits, hit_streak, age, det;
};
constexpr int TRACK_WORDS = sizeof(Track) / 8;
static_assert(sizeof(Track) == 224, "track layout");

struct StreamState {
  int32_t frame_count, n_tracks, ids_given, pad[5];
  Track tracks[MAXT];
};
static_assert(offsetof(StreamState, tracks) == 32, "state header");

struct Lsap {   // the per-row / per-column arrays of rectangular_lsap.cpp
  double u[64], v[64], spc[64];
  int col4row[64], row4col[64], path[64];
  unsigned char SR[64], SC[64];
};

// LDS traffic between the lanes of the one wave that solves the assignment
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

__device__ __forceinline__ double wave_min(double a) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const double b = __shfl_xor(a, m, 64);
    a = b < a ? b : a;
  }
  return a;
}

// linear_sum_assignment on cost[nr * nc], 0 < nr <= nc <= 64; col4row[i] = the column of row i.  Called by the whole of wave 0.
__device__ void lsap_wave(const double* cost, int nr, int nc, Lsap& w, int lane) {
  const double inf = __builtin_huge_val();
  if (lane < nr) { w.u[lane] = 0.0; w.col4row[lane] = -1; }
  if (lane < nc) { w.v[lane] = 0.0; w.row4col[lane] = -1; w.path[lane] = -1; }
  wave_sync();
  for (int cur = 0; cur < nr; ++cur) {
    // remaining[it] = nc - it - 1: lane `it` starts with that column
    const bool valid = lane < nc;
    int j = valid ? nc - 1 - lane : 0;
    double vj = valid ? w.v[j] : 0.0, spc = inf;
    int r4c = valid ? w.row4col[j] : 0;
    if (valid) w.SC[lane] = 0;
    if (lane < nr) w.SR[lane] = 0;
    wave_sync();
    double min_val = 0.0;
    int i = cur, num_remaining = nc, sink = -1;
    while (sink == -1) {
      if (lane == 0) w.SR[i] = 1;
      const bool act = lane < num_remaining;
      const double ui = w.u[i];
      if (act) {
        const double r = min_val + cost[i * nc + j] - ui - vj;
        if (r < spc) { w.path[j] = i; spc = r; }
      }
      const double lowest = wave_min(act ? spc : inf);
      const unsigned long long at_min = __ballot(act && spc == lowest);
      if (at_min == 0) return;   // infeasible: cannot happen with finite costs
      const int first = __ffsll((long long)at_min) - 1;
      const unsigned long long later_free = __ballot(act && spc == lowest && r4c == -1) & ~((2ull << first) - 1ull);
      const int index = later_free ? 63 - __clzll((long long)later_free) : first;
      min_val = lowest;
      const int jsel = __shfl(j, index, 64), rsel = __shfl(r4c, index, 64);
      if (lane == index) { w.spc[j] = spc; w.SC[j] = 1; }
      if (rsel == -1) sink = jsel; else i = rsel;
      // remaining[index] = remaining[--num_remaining]
      const int last = num_remaining - 1;
      const int j2 = __shfl(j, last, 64), r2 = __shfl(r4c, last, 64);
      const double v2 = __shfl(vj, last, 64), s2 = __shfl(spc, last, 64);
      if (lane == index) { j = j2; r4c = r2; vj = v2; spc = s2; }
      num_remaining = last;
    }
    wave_sync();
    if (lane == cur) w.u[cur] += min_val;
    else if (lane < nr && w.SR[lane]) w.u[lane] += min_val - w.spc[w.col4row[lane]];
    if (lane < nc && w.SC[lane]) w.v[lane] -= min_val - w.spc[lane];
    wave_sync();
    if (lane == 0) {
      int c = sink;
      for (int guard = 0; guard <= nr; ++guard) {
        const int r = w.path[c];
        w.row4col[c] = r;
        const int t = w.col4row[r];
        w.col4row[r] = c;
        c = t;
        if (r == cur) break;
      }
    }
    wave_sync();
  }
}

// one (coordinate, velocity) filter; p = the 2 x 2 block [a b; c d] row-major
__device__ __forceinline__ void kf_predict(double& pos, double& vel, double* p) {
  pos = pos + vel;
  const double a = p[0], b = p[1], c = p[2], d = p[3];
  const double fa = a + c, fb = b + d;               // F P, F = [1 1; 0 1]
  p[0] = (fa + fb) + 1.0;                            // (F P) F' + Q, Q = diag(1, 0.01)
  p[1] = fb;
  p[2] = c + d;
  p[3] = d + 0.01;
}
__device__ __forceinline__ void kf_update(double& pos, double& vel, double* p, double z, double rn) {
  const double a = p[0], b = p[1], c = p[2], d = p[3];
  const double y = z - pos;
  const double s = a + rn;
  const double k0 = a / s, k1 = c / s;               // K = P H' / S
  pos = pos + k0 * y;
  vel = vel + k1 * y;
  const double a00 = 1.0 - k0, a10 = -k1;            // A = I - K H = [a00 0; a10 1]
  const double m00 = a00 * a, m01 = a00 * b;         // A P
  const double m10 = a10 * a + c, m11 = a10 * b + d;
  p[0] = m00 * a00 + (k0 * rn) * k0;                 // (A P) A' + K R K'
  p[1] = (m00 * a10 + m01) + (k0 * rn) * k1;
  p[2] = m10 * a00 + (k1 * rn) * k0;
  p[3] = (m10 * a10 + m11) + (k1 * rn) * k1;
}

__global__ __launch_bounds__(THREADS) void box_tracks_kernel(me_box_tracks_desc d) {
  __shared__ double s_cost[MAXT * MAXD];   // -iou, rows = the smaller side
  __shared__ Track s_trk[MAXT];
  __shared__ float s_det[MAXD][7];
  __shared__ Lsap s_lsap;
  __shared__ int s_sum[THREADS];
  __shared__ int s_m_trk[MAXT], s_m_det[MAXD], s_newlist[MAXD], s_dst[MAXT], s_row[MAXT];
  __shared__ int s_status, s_n_new, s_n_alive, s_n_rows;

  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = d.streams;
  const int32_t* hd = reinterpret_cast<const int32_t*>(d.tail_out);
  const int head = (1 + 2 * S + 3) & ~3;
  const float* table = reinterpret_cast<const float*>(hd + head);
  StreamState* st = reinterpret_cast<StreamState*>(d.state) + s;
  int* cnt = d.counts + NCNT * s;

  // ---- this stream's rows in the tail's table: they start behind the rows of the streams before it ------------------------
  long long before = 0;
  int bad_counts = 0;
  for (int i = tid; i < s; i += THREADS) {
    const int c = hd[1 + i];
    if (c < 0 || c > d.m) bad_counts = 1; else before += c;
  }
  if (before > d.m) { bad_counts = 1; before = 0; }
  s_sum[tid] = (int)before;
  if (tid == 0) s_status = ME_TRACKS_OK;
  __syncthreads();
  for (int step = THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      const long long t = (long long)s_sum[tid] + s_sum[tid + step];
      s_sum[tid] = t > d.m ? d.m + 1 : (int)t;
    }
    __syncthreads();
  }
  const int row0 = s_sum[0];
  const int D = hd[1 + S + s];
  int T = st->n_tracks;
  if (T < 0 || T > MAXT) T = 0;   // (a state that was never reset)
  const int frame_count = st->frame_count, ids_given = st->ids_given;

  // ---- validate ----------------------------------------------------------------------------------------------------------
  int status = ME_TRACKS_OK;
  if (hd[0] != 0 || D < 0 || row0 > d.m || (long long)row0 + D > d.m) status = ME_TRACKS_E_INPUT;
  else if (D > MAXD) status = ME_TRACKS_E_DETS;
  if (__syncthreads_or(bad_counts) && status == ME_TRACKS_OK) status = ME_TRACKS_E_INPUT;
  int bad = 0;
  if (status == ME_TRACKS_OK && tid < D) {
    const float* q = table + (size_t)(row0 + tid) * 7;
    for (int c = 0; c < 7; ++c) s_det[tid][c] = q[c];
    for (int c = 0; c < 4; ++c) bad |= !(fabsf(q[c]) <= 3.4028234e38f);
  }
  if (__syncthreads_or(bad) && status == ME_TRACKS_OK) status = ME_TRACKS_E_INPUT;
  if (status != ME_TRACKS_OK) {   // uniform; nothing of the state has been written
    if (tid == 0) { cnt[0] = status; cnt[1] = 0; cnt[2] = T; cnt[3] = frame_count; }
    return;
  }

  // ---- LDS copy of the tracks; predict --------------------------------------------------------------------------------------
  for (int e = tid; e < T * TRACK_WORDS; e += THREADS)
    reinterpret_cast<unsigned long long*>(s_trk)[e] = reinterpret_cast<const unsigned long long*>(st->tracks)[e];
  if (tid < MAXT) s_m_trk[tid] = -1;
  if (tid < MAXD) s_m_det[tid] = -1;
  __syncthreads();
  if (tid < T) {
    Track& t = s_trk[tid];
    if (t.x[2] + t.x[6] <= 0.0) t.x[6] = 0.0;
    if (t.x[3] + t.x[7] <= 0.0) t.x[7] = 0.0;
    for (int c = 0; c < 4; ++c) kf_predict(t.x[c], t.x[c + 4], t.P[c]);
    if (t.time_since_update > 0) t.hit_streak = 0;
    t.time_since_update += 1;
    t.age += 1;
  }
  __syncthreads();

  // ---- IoU of every predicted box with every detection ------------------------------------------------------------------------
  const bool tracks_are_rows = T <= D;   // scipy transposes a matrix with more rows than columns
  for (int e = tid; e < T * D; e += THREADS) {
    const int i = e / D, j = e - i * D;
    const Track& t = s_trk[i];
    const double tx1 = t.x[0] - t.x[2] / 2.0, ty1 = t.x[1] - t.x[3] / 2.0;
    const double tx2 = t.x[0] + t.x[2] / 2.0, ty2 = t.x[1] + t.x[3] / 2.0;
    const double dx1 = (double)s_det[j][0], dy1 = (double)s_det[j][1], dx2 = (double)s_det[j][2], dy2 = (double)s_det[j][3];
    const double ix1 = tx1 > dx1 ? tx1 : dx1, iy1 = ty1 > dy1 ? ty1 : dy1;
    const double ix2 = tx2 < dx2 ? tx2 : dx2, iy2 = ty2 < dy2 ? ty2 : dy2;
    const double iw = ix2 - ix1, ih = iy2 - iy1;
    double iou = 0.0;
    if (iw > 0.0 && ih > 0.0 && t.cls == s_det[j][6]) {
      const double inter = iw * ih;
      const double area_t = (tx2 - tx1) * (ty2 - ty1), area_d = (dx2 - dx1) * (dy2 - dy1);
      iou = inter / ((area_t + area_d) - inter);
    }
    if (tracks_are_rows) s_cost[i * D + j] = -iou; else s_cost[j * T + i] = -iou;
  }
  __syncthreads();

  // ---- exact assignment (wave 0), the iou_min gate, the births ------------------------------------------------------------------
  if (wave == 0) {
    if (T > 0 && D > 0) {
      if (tracks_are_rows) lsap_wave(s_cost, T, D, s_lsap, lane); else lsap_wave(s_cost, D, T, s_lsap, lane);
      const int nr = tracks_are_rows ? T : D, nc = tracks_are_rows ? D : T;
      if (lane < nr) {
        const int c = s_lsap.col4row[lane];
        if (c >= 0 && -s_cost[lane * nc + c] >= d.iou_min) {
          const int i = tracks_are_rows ? lane : c, j = tracks_are_rows ? c : lane;
          s_m_trk[i] = j;
          s_m_det[j] = i;
        }
      }
      wave_sync();
    }
    if (lane == 0) {
      int n_new = 0;
      for (int j = 0; j < D; ++j)
        if (s_m_det[j] < 0 && (double)s_det[j][4] >= d.birth_conf) s_newlist[n_new++] = j;
      if (T + n_new > MAXT) s_status = ME_TRACKS_E_TRACKS;
      s_n_new = n_new;
    }
  }
  __syncthreads();
  if (s_status != ME_TRACKS_OK) {   // nothing of the state has been written
    if (tid == 0) { cnt[0] = s_status; cnt[1] = 0; cnt[2] = T; cnt[3] = frame_count; }
    return;
  }
  if (d.matches && tid < T) d.matches[(size_t)s * MAXT + tid] = s_m_trk[tid];
  if (d.cost)
    for (int e = tid; e < T * D; e += THREADS) {
      const int i = e / D, j = e - i * D;
      d.cost[((size_t)s * MAXT + i) * MAXD + j] = -(tracks_are_rows ? s_cost[i * D + j] : s_cost[j * T + i]);
    }

  // ---- update the matched tracks, append the births ----------------------------------------------------------------------------
  const int n_new = s_n_new;
  if (tid < T && s_m_trk[tid] >= 0) {
    Track& t = s_trk[tid];
    const int j = s_m_trk[tid];
    const double x1 = (double)s_det[j][0], y1 = (double)s_det[j][1], x2 = (double)s_det[j][2], y2 = (double)s_det[j][3];
    const double z[4] = {(x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1};
    for (int c = 0; c < 4; ++c) kf_update(t.x[c], t.x[c + 4], t.P[c], z[c], c < 2 ? 1.0 : 10.0);
    t.time_since_update = 0;
    t.hits += 1;
    t.hit_streak += 1;
    t.conf = s_det[j][4];
    t.det = j;
  }
  if (tid >= MAXT && tid - MAXT < n_new) {   // (T + n_new <= MAXT)
    const int k = tid - MAXT, j = s_newlist[k];
    Track& t = s_trk[T + k];
    const double x1 = (double)s_det[j][0], y1 = (double)s_det[j][1], x2 = (double)s_det[j][2], y2 = (double)s_det[j][3];
    t.x[0] = (x1 + x2) / 2.0; t.x[1] = (y1 + y2) / 2.0; t.x[2] = x2 - x1; t.x[3] = y2 - y1;
    for (int c = 0; c < 4; ++c) {
      t.x[c + 4] = 0.0;
      t.P[c][0] = 10.0; t.P[c][1] = 0.0; t.P[c][2] = 0.0; t.P[c][3] = 1e4;
    }
    t.id = ids_given + k + 1;
    t.cls = s_det[j][6];
    t.conf = s_det[j][4];
    t.time_since_update = 0; t.hits = 0; t.hit_streak = 0; t.age = 0;
    t.det = j;
  }
  __syncthreads();

  // ---- deaths (order kept), the output rule, commit ----------------------------------------------------------------------------
  const int Tn = T + n_new, fc = frame_count + 1;
  if (tid == 0) {
    int alive = 0, rows = 0;
    for (int k = 0; k < Tn; ++k) {
      const Track& t = s_trk[k];
      s_row[k] = -1;
      if (t.time_since_update > d.max_age) { s_dst[k] = -1; continue; }
      if (t.time_since_update == 0 && (t.hit_streak >= d.min_hits || fc <= d.min_hits)) s_row[k] = rows++;
      s_dst[k] = alive++;
    }
    s_n_alive = alive;
    s_n_rows = rows;
  }
  __syncthreads();
  for (int e = tid; e < Tn * TRACK_WORDS; e += THREADS) {
    const int k = e / TRACK_WORDS, wd = e - k * TRACK_WORDS, dst = s_dst[k];
    if (dst >= 0)
      reinterpret_cast<unsigned long long*>(st->tracks + dst)[wd] = reinterpret_cast<const unsigned long long*>(s_trk + k)[wd];
  }
  if (tid < Tn && s_row[tid] >= 0) {
    const Track& t = s_trk[tid];
    double* o = d.tracks + ((size_t)s * MAXT + s_row[tid]) * ROWC;
    o[0] = (double)t.id;
    o[1] = t.x[0] - t.x[2] / 2.0; o[2] = t.x[1] - t.x[3] / 2.0;
    o[3] = t.x[0] + t.x[2] / 2.0; o[4] = t.x[1] + t.x[3] / 2.0;
    o[5] = (double)t.conf; o[6] = (double)t.cls;
    o[7] = (double)t.hit_streak; o[8] = (double)t.age; o[9] = (double)t.det;
  }
  if (tid == 0) {
    st->frame_count = fc;
    st->n_tracks = s_n_alive;
    st->ids_given = ids_given + n_new;
    cnt[0] = ME_TRACKS_OK; cnt[1] = s_n_rows; cnt[2] = s_n_alive; cnt[3] = fc;
  }
}

}  // namespace

extern "C" {

int32_t me_box_tracks_capacity(int32_t which) {
  switch (which) {
    case 0: return MAXD;
    case 1: return MAXT;
    case 2: return ROWC;
    case 3: return NCNT;
    case 4: return (int32_t)offsetof(StreamState, tracks);
    case 5: return (int32_t)sizeof(Track);
    default: return -1;
  }
}

int64_t me_box_tracks_state_bytes(int32_t streams) { return streams > 0 ? (int64_t)streams * (int64_t)sizeof(StreamState) : 0; }

int me_box_tracks_reset(void* state, int32_t streams, int32_t which, void* stream) {
  ME_REQUIRE(state, ME_E_NULLPTR, "me_box_tracks_reset: null pointer");
  ME_REQUIRE(streams > 0 && which < streams, ME_E_BADARG, "me_box_tracks_reset: stream %d of %d", which, streams);
  StreamState* st = reinterpret_cast<StreamState*>(state);
  if (which < 0)
    ME_HIP(hipMemsetAsync(st, 0, sizeof(StreamState) * (size_t)streams, (hipStream_t)stream));
  else
    ME_HIP(hipMemsetAsync(st + which, 0, sizeof(StreamState), (hipStream_t)stream));
  return 0;
}

int me_box_tracks_f64(const me_box_tracks_desc* d, void* stream) {
  ME_REQUIRE(d, ME_E_NULLPTR, "me_box_tracks_f64: null descriptor");
  ME_REQUIRE(d->tail_out && d->state && d->tracks && d->counts, ME_E_NULLPTR, "me_box_tracks_f64: null pointer");
  ME_REQUIRE(d->streams > 0 && d->streams <= 65535 && d->m >= 0, ME_E_BADARG, "me_box_tracks_f64: %d streams, m = %d",
             d->streams, d->m);
  ME_REQUIRE(d->max_age >= 0 && d->min_hits >= 0 && d->iou_min == d->iou_min && d->birth_conf == d->birth_conf, ME_E_BADARG,
             "me_box_tracks_f64: bad tracker parameters");
  ME_REQUIRE(me::aligned16(d->tail_out) && me::aligned16(d->state), ME_E_ALIGN,
             "me_box_tracks_f64: tail_out / state not 16-byte aligned");
  hipLaunchKernelGGL(box_tracks_kernel, dim3(d->streams), dim3(THREADS), 0, (hipStream_t)stream, *d);
  return me::check_launch("box_tracks_kernel");
}

}  // extern "C"
