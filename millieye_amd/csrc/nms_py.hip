// nms_py.hip - the reference's Python NMS (+1-pixel IoU, label equality, no cap on kept boxes, optional box merging) on the
// GPU (gfx950).
//
// Replaces, bit for bit in every decision and in columns 4-6:
//   non_max_suppression  module3_our_dataset/utils/utils.py:281-334 (= module2_mixed/utils/utils.py, one comment apart):
//                        rank by objectness, remove when iou > thr, boxes unchanged            (score_mode 0, inclusive 0, merge 0)
//   non_max_suppression  module3_our_dataset/yolov3/utils/utils.py:231-293 (the vendored PyTorch-YOLOv3 function): rank by
//                        obj * cls_conf, remove when iou >= thr, the keeper's box becomes the objectness-weighted mean of the
//                        boxes it removes, itself included                                     (score_mode 1, inclusive 1, merge 1)
// with bbox_iou (utils/utils.py:248-278) and xywh2xyxy (:68-74) in fp32, contraction off, in the reference's operation order:
//   inter = max(min(x2) - max(x1) + 1, 0) * max(min(y2) - max(y1) + 1, 0),  area = (x2 - x1 + 1) * (y2 - y1 + 1),
//   iou = inter / (((a_i + a_j) - inter) + 1e-16f);  a NaN anywhere makes the test false (torch.max / min / clamp propagate it).
// Ties of the score go to the lower row first (the reference's argsort is unstable there; the rule of nms.hip).
//
// ONE DEPARTURE from the reference: the keeper always removes itself.  The reference loops forever when the top box fails its own
// test (a NaN coordinate, w + 1 <= 0, thr >= 1: `detections = detections[~invalid]` then never shrinks); here such a box is kept
// once and, under merging, is its own cluster of one.
//
// The greedy walk, restated: with the candidates sorted, owner[j] = the first keeper i < j with label_i == label_j whose IoU with j
// passes the test; j is a keeper exactly when there is none.  A keeper's merge cluster is itself plus every j it owns (the
// reference removes j at the turn of the FIRST keeper that matches it, and tests with the un-merged boxes).  Nothing in this needs
// one workgroup to walk the whole list:
//   pynms_prep    one thread per row: xywh -> xyxy in place, obj >= conf_thresh filter, class max / argmax (torch.max(1) rule:
//                 cls_beats of nms.hip), score, candidate append (one global integer atomic per workgroup)
//   pynms_rank    sorted position = number of larger (score, ~row) keys; writes the sorted box / obj / cls_conf / label arrays
//   pynms_diag    every tile of TILE sorted candidates: the TILE x TILE bit matrix "i removes j" (j > i, same label, IoU passes),
//                 all tiles of all images in one launch, a wave per 64 x 64 block
//   per tile k, in order (ceil(rows / TILE) rounds; a round past the image's candidates returns at once):
//     pynms_cross   (k > 0) whole chip: candidate j of tile k against the keepers of tiles < k, KCHUNK keepers per workgroup
//                   staged in LDS; owner[j] = atomicMin of the matching keepers' sorted positions (an integer minimum: the result
//                   does not depend on the order of the atomics)
//     pynms_tile    one workgroup per image: the tile's matrix rows in LDS (128 KiB), wave 0 walks the candidates no earlier
//                   keeper owns (find-first-set on the not-removed word, OR the keeper's row in - the machinery of nms_scan),
//                   then every removed candidate finds its first keeper of the tile in the matrix column; keepers are appended
//                   to the image's keeper list
//   pynms_emit    a wave per kept row: box (merge: sum of obj * box and of obj over the cluster in float64, lane l takes members
//                 l, l + 64, ... in ascending order, then a fixed shuffle tree - no floating-point atomics, the same bits on every
//                 call), obj, cls_conf, label
// Capacity: rows <= 32768, every row may be a candidate and every candidate a keeper.
#include <math.h>
#include "common.h"

namespace {

constexpr int PY_MAX_ROWS = 32768;
constexpr int TILE = 1024;         // sorted candidates per round (hip.PYNMS_TILE)
constexpr int TW = TILE / 64;      // 64-bit words per matrix row
constexpr int KCHUNK = 256;        // earlier keepers per pynms_cross workgroup (hip.PYNMS_KEEPER_CHUNK)
constexpr int NO_OWNER = 0x7fffffff;

struct PyWs {
  float4* ubox;              // [n][cap] candidates in append order: xyxy
  unsigned long long* ukey;  // [n][cap] (sortable(score) << 32) | ~row
  float* uobj;               // [n][cap]
  float* ucls;               // [n][cap]
  float* ulab;               // [n][cap]
  float4* sbox;              // [n][cap] the same in sorted order
  float* sobj;
  float* scls;
  float* slab;
  int* owner;                // [n][cap] sorted position of the keeper that removes the candidate (keepers: their own), NO_OWNER
  int* nmemb;                // [n][cap] merge: number of candidates a keeper owns besides itself
  int* kpos;                 // [n][cap] sorted positions of the keepers, in order
  unsigned long long* mat;   // [n][cap][TW] row i of its tile's bit matrix
  int* cand_count;           // [n]
  int* kcount;               // [n]
  int cap;
};

inline long long up256(long long v) { return (v + 255) / 256 * 256; }

inline long long py_ws_bytes(int n, int rows) {
  const long long e = (long long)n * rows;
  return up256(e * 16) * 2 + up256(e * 8) + up256(e * 4) * 9 + up256(e * TW * 8) + up256((long long)n * 8);
}

inline PyWs py_carve(void* base, int n, int rows) {
  PyWs w;
  char* p = reinterpret_cast<char*>(base);
  const long long e = (long long)n * rows;
  w.cap = rows;
  w.ubox = reinterpret_cast<float4*>(p); p += up256(e * 16);
  w.sbox = reinterpret_cast<float4*>(p); p += up256(e * 16);
  w.ukey = reinterpret_cast<unsigned long long*>(p); p += up256(e * 8);
  w.uobj = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.ucls = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.ulab = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.sobj = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.scls = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.slab = reinterpret_cast<float*>(p); p += up256(e * 4);
  w.owner = reinterpret_cast<int*>(p); p += up256(e * 4);
  w.nmemb = reinterpret_cast<int*>(p); p += up256(e * 4);
  w.kpos = reinterpret_cast<int*>(p); p += up256(e * 4);
  w.mat = reinterpret_cast<unsigned long long*>(p); p += up256(e * TW * 8);
  w.cand_count = reinterpret_cast<int*>(p);
  w.kcount = w.cand_count + n;
  return w;
}

__device__ __forceinline__ unsigned py_sortable(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// torch.max(1): any NaN beats every number (the first NaN wins), otherwise the larger value, ties to the lower index
__device__ __forceinline__ bool py_cls_beats(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ float py_area(const float4 b) {
#pragma clang fp contract(off)
  return ((b.z - b.x) + 1.f) * ((b.w - b.y) + 1.f);
}

__device__ __forceinline__ bool py_has_nan(const float4 b) { return (b.x != b.x) | (b.y != b.y) | (b.z != b.z) | (b.w != b.w); }

// bbox_iou(keeper, candidate) > thr (inclusive: >= thr); the areas are py_area of the two boxes
__device__ __forceinline__ bool py_iou_passes(const float4 bi, float ai, const float4 bj, float aj, float thr, int inclusive) {
#pragma clang fp contract(off)
  if (py_has_nan(bi) || py_has_nan(bj)) return false;  // torch.max / min / clamp hand a NaN on: the IoU is NaN, the test false
  const float x1 = fmaxf(bi.x, bj.x), y1 = fmaxf(bi.y, bj.y);
  const float x2 = fminf(bi.z, bj.z), y2 = fminf(bi.w, bj.w);
  const float dw = (x2 - x1) + 1.f, dh = (y2 - y1) + 1.f;
  if (dw != dw || dh != dh) return false;  // (inf - inf)
  const float inter = (dw < 0.f ? 0.f : dw) * (dh < 0.f ? 0.f : dh);
  const float iou = inter / (((ai + aj) - inter) + 1e-16f);
  return inclusive ? iou >= thr : iou > thr;
}

__global__ __launch_bounds__(256) void pynms_zero_kernel(int* p, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) p[i] = 0;
}

// ---- prep ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pynms_prep_kernel(float* pred, int rows, int num_classes, float conf_thresh, int score_mode,
                                                         int writeback, PyWs w) {
#pragma clang fp contract(off)
  __shared__ int s_rows[256];
  __shared__ int s_n, s_base;
  const int img = blockIdx.y;
  const int row = blockIdx.x * 256 + threadIdx.x;
  const int per = 5 + num_classes;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  if (row < rows) {
    float* p = pred + ((long long)img * rows + row) * per;
    const float conf = p[4];
    if (writeback) {  // xywh2xyxy (utils.py:68-74) in place on every row: half extents as w / 2
      const float cx = p[0], cy = p[1], bw = p[2], bh = p[3];
      p[0] = cx - bw / 2; p[1] = cy - bh / 2; p[2] = cx + bw / 2; p[3] = cy + bh / 2;
    }
    if (conf >= conf_thresh) s_rows[atomicAdd(&s_n, 1)] = row;  // (a NaN objectness fails; order: the key carries the row)
  }
  __syncthreads();
  const int npass = s_n;
  if (npass == 0) return;
  if (threadIdx.x == 0) s_base = atomicAdd(&w.cand_count[img], npass);
  __syncthreads();
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;  // 16 lanes per passing row read its class scores
  for (int q = grp; q < npass; q += 16) {
    const int r = s_rows[q];
    const float* p = pred + ((long long)img * rows + r) * per;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = gl; c < num_classes; c += 16) {
      const float v = p[5 + c];
      if (arg == 0x7fffffff || py_cls_beats(v, c, best, arg)) {
        best = v;
        arg = c;
      }
    }
#pragma unroll
    for (int sft = 8; sft >= 1; sft >>= 1) {
      const float ov = __shfl_xor(best, sft, 16);
      const int oi = __shfl_xor(arg, sft, 16);
      if (oi != 0x7fffffff && (arg == 0x7fffffff || py_cls_beats(ov, oi, best, arg))) {
        best = ov;
        arg = oi;
      }
    }
    if (gl == 0) {
      if (arg == 0x7fffffff) arg = 0;  // (no classes)
      float x1, y1, x2, y2;
      if (writeback) {  // converted above (same workgroup, behind the barrier)
        x1 = p[0]; y1 = p[1]; x2 = p[2]; y2 = p[3];
      } else {
        const float cx = p[0], cy = p[1], bw = p[2], bh = p[3];
        x1 = cx - bw / 2; y1 = cy - bh / 2; x2 = cx + bw / 2; y2 = cy + bh / 2;
      }
      const float obj = p[4];
      const float score = (score_mode ? obj * best : obj) + 0.f;  // (+ 0: -0 and +0 are one score)
      const long long o = (long long)img * w.cap + s_base + q;
      w.ubox[o] = make_float4(x1, y1, x2, y2);
      w.ukey[o] = ((unsigned long long)py_sortable(score) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)r);
      w.uobj[o] = obj;
      w.ucls[o] = best;
      w.ulab[o] = (float)arg;
    }
  }
}

// ---- rank ---------------------------------------------------------------------------------------------------------------------
constexpr int PY_RANK_TILE = 2048;
__global__ __launch_bounds__(256) void pynms_rank_kernel(PyWs w) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_keys[PY_RANK_TILE];
  const int img = blockIdx.y;
  const int cnt = w.cand_count[img];
  if ((int)blockIdx.x * 256 >= cnt) return;
  const long long base = (long long)img * w.cap;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long mine = j < cnt ? w.ukey[base + j] : ~0ull;
  int rank = 0;
  for (int t0 = 0; t0 < cnt; t0 += PY_RANK_TILE) {
    const int len = cnt - t0 < PY_RANK_TILE ? cnt - t0 : PY_RANK_TILE;
    __syncthreads();
    for (int i = threadIdx.x; i < PY_RANK_TILE; i += 256) s_keys[i] = i < len ? w.ukey[base + t0 + i] : 0ull;  // 0 < every key
    __syncthreads();
    const int len2 = (len + 1) & ~1;
    for (int i = 0; i < len2; i += 2) {
      const ulonglong2 k2 = *reinterpret_cast<const ulonglong2*>(&s_keys[i]);
      rank += (k2.x > mine ? 1 : 0) + (k2.y > mine ? 1 : 0);
    }
  }
  if (j >= cnt) return;  // keys are unique (they embed the row): rank is a permutation of 0 .. cnt - 1
  w.sbox[base + rank] = w.ubox[base + j];
  w.sobj[base + rank] = w.uobj[base + j];
  w.scls[base + rank] = w.ucls[base + j];
  w.slab[base + rank] = w.ulab[base + j];
  w.owner[base + rank] = NO_OWNER;
  w.nmemb[base + rank] = 0;
}

// ---- the tiles' own bit matrices ---------------------------------------------------------------------------------------------------
// workgroup = (image, tile, block of 64 rows); wave v takes the words v, v + 4, ... of those rows (lane = row, the 64 column
// candidates broadcast by readlane).  Words left of the diagonal are written as 0: the workspace holds anything on entry.
__global__ __launch_bounds__(256) void pynms_diag_kernel(PyWs w, float thr, int inclusive) {
#pragma clang fp contract(off)
  const int img = blockIdx.y;
  const int cnt = w.cand_count[img];
  const int tile = blockIdx.x / TW, rb = blockIdx.x - tile * TW;
  const int t0 = tile * TILE;
  const int row0 = t0 + rb * 64;
  if (row0 >= cnt) return;
  const long long base = (long long)img * w.cap;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = row0 + lane;
  float4 rbx = make_float4(0.f, 0.f, 0.f, 0.f);
  float rl = -1.f;
  if (row < cnt) {
    rbx = w.sbox[base + row];
    rl = w.slab[base + row];
  }
  const float ra = py_area(rbx);
  for (int cw = wv; cw < TW; cw += 4) {
    unsigned long long bits = 0ull;
    const int col0 = t0 + cw * 64;
    if (cw >= rb && col0 < cnt) {  // (uniform per wave)
      const int col = col0 + lane;
      float4 cb = make_float4(0.f, 0.f, 0.f, 0.f);
      float cl = -2.f;
      if (col < cnt) {
        cb = w.sbox[base + col];
        cl = w.slab[base + col];
      }
      const float ca = py_area(cb);
      for (int b = 0; b < 64; ++b) {
        float4 bj;
        bj.x = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(cb.x), b));
        bj.y = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(cb.y), b));
        bj.z = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(cb.z), b));
        bj.w = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(cb.w), b));
        const float ja = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(ca), b));
        const float jl = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(cl), b));
        const int j = col0 + b;
        if (j > row && j < cnt && row < cnt && jl == rl && py_iou_passes(rbx, ra, bj, ja, thr, inclusive)) bits |= 1ull << b;
      }
    }
    if (row < cnt) w.mat[(base + row) * TW + cw] = bits;
  }
}

// ---- cross: tile k against the keepers of the tiles before it ------------------------------------------------------------------------
// grid (keeper chunk, TILE / 256 blocks of candidates, image).  The keepers of a chunk are in ascending sorted position, so the
// first match of a thread is its minimum of the chunk.
__global__ __launch_bounds__(256) void pynms_cross_kernel(PyWs w, int tile, float thr, int inclusive) {
#pragma clang fp contract(off)
  __shared__ float4 s_box[KCHUNK];
  __shared__ float s_area[KCHUNK], s_lab[KCHUNK];
  __shared__ int s_pos[KCHUNK];
  const int img = blockIdx.z;
  const int cnt = w.cand_count[img];
  const int t0 = tile * TILE;
  const int j0 = t0 + blockIdx.y * 256;
  if (j0 >= cnt) return;
  const int kc = w.kcount[img];  // every keeper so far sits in an earlier tile
  const int k0 = blockIdx.x * KCHUNK;
  if (k0 >= kc) return;
  const int klen = kc - k0 < KCHUNK ? kc - k0 : KCHUNK;
  const long long base = (long long)img * w.cap;
  if ((int)threadIdx.x < klen) {
    const int pos = w.kpos[base + k0 + threadIdx.x];
    const float4 b = w.sbox[base + pos];
    s_pos[threadIdx.x] = pos;
    s_box[threadIdx.x] = b;
    s_area[threadIdx.x] = py_area(b);
    s_lab[threadIdx.x] = w.slab[base + pos];
  }
  __syncthreads();
  const int j = j0 + threadIdx.x;
  if (j >= cnt) return;
  const float4 bj = w.sbox[base + j];
  const float aj = py_area(bj), lj = w.slab[base + j];
  for (int q = 0; q < klen; ++q) {
    if (s_lab[q] == lj && py_iou_passes(s_box[q], s_area[q], bj, aj, thr, inclusive)) {
      atomicMin(&w.owner[base + j], s_pos[q]);
      break;
    }
  }
}

// ---- tile: the walk inside tile k ---------------------------------------------------------------------------------------------
constexpr int TILE_THREADS = 1024;
constexpr size_t kTileLds = (size_t)TILE * TW * 8 + TILE * 4 + TW * 8 + 16;  // matrix rows, keeper list, keeper bits, {kept, kbase}

__global__ __launch_bounds__(TILE_THREADS) void pynms_tile_kernel(PyWs w, int tile, int merge) {
  extern __shared__ __attribute__((aligned(16))) unsigned char py_lds[];
  unsigned long long* s_mat = reinterpret_cast<unsigned long long*>(py_lds);                       // [TILE][TW]
  int* s_keep = reinterpret_cast<int*>(py_lds + (size_t)TILE * TW * 8);                           // [TILE] positions in the tile
  unsigned long long* s_kbits = reinterpret_cast<unsigned long long*>(py_lds + (size_t)TILE * TW * 8 + TILE * 4);  // [TW]
  int* s_misc = reinterpret_cast<int*>(py_lds + (size_t)TILE * TW * 8 + TILE * 4 + TW * 8);       // kept, kbase
  const int img = blockIdx.x;
  const int cnt = w.cand_count[img];
  const int t0 = tile * TILE;
  if (t0 >= cnt) return;
  const int len = cnt - t0 < TILE ? cnt - t0 : TILE;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long base = (long long)img * w.cap;
  // the tile's matrix rows: 16-byte pieces, rows at or past len as zeros (pynms_diag did not write them)
  {
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(w.mat + (base + t0) * TW);
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(s_mat);
    constexpr int PIECES = TILE * TW / 2, PER_ROW = TW / 2;
    for (int p = t; p < PIECES; p += TILE_THREADS) dst[p] = (p / PER_ROW < len) ? src[p] : make_ulonglong2(0ull, 0ull);
  }
  // removed so far: owned by a keeper of an earlier tile (pynms_cross), or past the end; wave v builds word v
  const int own_in = t < len ? w.owner[base + t0 + t] : 0;
  const unsigned long long gone = __builtin_amdgcn_ballot_w64(t >= len || own_in != NO_OWNER);
  if (lane == 0) s_kbits[wv] = gone;  // (staging: replaced by the keeper bits below)
  if (t == 0) s_misc[1] = w.kcount[img];
  __syncthreads();
  if (wv == 0) {
    unsigned long long rem = lane < TW ? s_kbits[lane] : ~0ull;
    unsigned long long kb = 0ull;
    int kept = 0, i = 0;
    while (i < len) {
      const int wd = i >> 6;
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rem, wd);
      const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rem >> 32), wd);
      unsigned long long avail = ~(((unsigned long long)hi << 32) | lo);
      avail &= ~0ull << (i & 63);
      if (avail == 0ull) {
        i = (wd + 1) << 6;
        continue;
      }
      const int bit = __builtin_ctzll(avail);
      i = (wd << 6) + bit;  // < len: the bits at and past len are set in rem
      if (lane == 0) s_keep[kept] = i;
      ++kept;
      if (lane == wd) kb |= 1ull << bit;
      if (lane < TW) rem |= s_mat[(size_t)i * TW + lane];
      ++i;
    }
    if (lane < TW) s_kbits[lane] = kb;
    if (lane == 0) s_misc[0] = kept;
  }
  __syncthreads();
  const int kept = s_misc[0], kbase = s_misc[1];
  if (t < len) {
    int own = own_in;
    if (own == NO_OWNER) {
      if ((s_kbits[wv] >> lane) & 1ull) {
        own = t0 + t;  // a keeper owns itself
      } else {
        for (int q = 0; q < kept; ++q) {  // removed inside the tile: the first keeper whose row holds this column
          const int i = s_keep[q];
          if (i >= t) break;
          if ((s_mat[(size_t)i * TW + wv] >> lane) & 1ull) {
            own = t0 + i;
            break;
          }
        }
      }
      w.owner[base + t0 + t] = own;
    }
    if (merge && own != t0 + t && own != NO_OWNER) atomicAdd(&w.nmemb[base + own], 1);
  }
  for (int q = t; q < kept; q += TILE_THREADS) w.kpos[base + kbase + q] = t0 + s_keep[q];
  if (t == 0) w.kcount[img] = kbase + kept;
}

inline hipError_t tile_lds_attr() {  // > 64 KiB of dynamic LDS needs the opt-in, once per process
  static hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(pynms_tile_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileLds);
  return rc;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------
// a wave per kept row.  merge: the cluster = the keeper and every candidate it owns; the members lie behind it in sorted order.
__global__ __launch_bounds__(256) void pynms_emit_kernel(PyWs w, int rows, int merge, float* det, int* count) {
  const int img = blockIdx.y;
  const int kc = w.kcount[img];
  const int cnt = w.cand_count[img];
  if (blockIdx.x == 0 && threadIdx.x == 0) count[img] = cnt > 0 ? kc : 0;
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cnt <= 0 || q >= kc) return;
  const long long base = (long long)img * w.cap;
  const int pos = w.kpos[base + q];
  float4 box = w.sbox[base + pos];
  if (merge) {
    // sum(w * box) / sum(w), w = obj (yolov3/utils/utils.py:284-287) in float64: a product of two floats is exact there
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0, so = 0.0;
    if (w.nmemb[base + pos] > 0) {
      for (int j = pos + lane; j < cnt; j += 64) {
        if (w.owner[base + j] == pos) {
          const float4 b = w.sbox[base + j];
          const double o = (double)w.sobj[base + j];
          sx += o * (double)b.x; sy += o * (double)b.y; sz += o * (double)b.z; sw += o * (double)b.w;
          so += o;
        }
      }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        sx += __shfl_xor(sx, s, 64); sy += __shfl_xor(sy, s, 64); sz += __shfl_xor(sz, s, 64); sw += __shfl_xor(sw, s, 64);
        so += __shfl_xor(so, s, 64);
      }
    } else {
      const double o = (double)w.sobj[base + pos];
      sx = o * (double)box.x; sy = o * (double)box.y; sz = o * (double)box.z; sw = o * (double)box.w;
      so = o;
    }
    box = make_float4((float)(sx / so), (float)(sy / so), (float)(sz / so), (float)(sw / so));
  }
  if (lane == 0) {
    float* out = det + ((long long)img * rows + q) * 7;
    out[0] = box.x; out[1] = box.y; out[2] = box.z; out[3] = box.w;
    out[4] = w.sobj[base + pos];
    out[5] = w.scls[base + pos];
    out[6] = w.slab[base + pos];
  }
}

}  // namespace

extern "C" {

int64_t me_nms_python_workspace_bytes(int32_t n, int32_t rows) {
  if (n <= 0 || rows <= 0 || rows > PY_MAX_ROWS) return 0;
  return py_ws_bytes(n, rows);
}

int me_nms_python_f32(const me_nms_python_desc* d, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  ME_REQUIRE(d && d->pred && d->det && d->count && d->workspace, ME_E_NULLPTR, "me_nms_python_f32: null pointer");
  ME_REQUIRE(d->n > 0 && d->rows > 0 && d->num_classes >= 0, ME_E_BADARG, "me_nms_python_f32: bad dimensions");
  ME_REQUIRE(d->rows <= PY_MAX_ROWS, ME_E_TOOBIG, "me_nms_python_f32: rows %d > capacity %d", d->rows, PY_MAX_ROWS);
  ME_REQUIRE(d->n <= 65535, ME_E_TOOBIG, "me_nms_python_f32: batch too large");
  ME_REQUIRE((reinterpret_cast<uintptr_t>(d->workspace) & 255u) == 0, ME_E_ALIGN,
             "me_nms_python_f32: workspace not 256-byte aligned");
  const int n = d->n, rows = d->rows;
  const int inclusive = d->inclusive ? 1 : 0, merge = d->merge ? 1 : 0;
  PyWs w = py_carve(d->workspace, n, rows);
  hipLaunchKernelGGL(pynms_zero_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, stream, w.cand_count, 2 * n);
  hipLaunchKernelGGL(pynms_prep_kernel, dim3((rows + 255) / 256, n), dim3(256), 0, stream, d->pred, rows, d->num_classes,
                     d->conf_thresh, d->score_mode ? 1 : 0, d->writeback_xyxy ? 1 : 0, w);
  int rc = me::check_launch("pynms_prep_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(pynms_rank_kernel, dim3((rows + 255) / 256, n), dim3(256), 0, stream, w);
  const int tiles = (rows + TILE - 1) / TILE;
  hipLaunchKernelGGL(pynms_diag_kernel, dim3(tiles * TW, n), dim3(256), 0, stream, w, d->iou_thresh, inclusive);
  rc = me::check_launch("pynms_diag_kernel");
  if (rc) return rc;
  ME_HIP(tile_lds_attr());
  for (int k = 0; k < tiles; ++k) {
    if (k > 0)  // at most k * TILE keepers so far
      hipLaunchKernelGGL(pynms_cross_kernel, dim3(k * TILE / KCHUNK, TILE / 256, n), dim3(256), 0, stream, w, k, d->iou_thresh,
                         inclusive);
    hipLaunchKernelGGL(pynms_tile_kernel, dim3(n), dim3(TILE_THREADS), kTileLds, stream, w, k, merge);
    rc = me::check_launch("pynms_tile_kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pynms_emit_kernel, dim3((rows + 3) / 4, n), dim3(256), 0, stream, w, rows, merge, d->det, d->count);
  return me::check_launch("pynms_emit_kernel");
}

}  // extern "C"
