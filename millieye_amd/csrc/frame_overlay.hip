// Boxes and labels painted into the pictures of S independent streams: what millieye_amd/frame_overlay.py:draw_detections
// does per frame on the host, behind me_stream_tail_f32 (csrc/nms.hip), me_box_tracks_f64 and me_box_ranges_f64 and read
// straight from their device buffers.
//   frame_overlay_kernel   grid (stream, chunk): validate the tail's words and the stream's surface -> wave 0 lists the drawn
//                          rows in order -> one thread per drawn row builds its box item and its label item (corners, colour,
//                          track id, label text) in LDS -> the chunks of a stream stride over the items; the workgroup walks the
//                          pixels of an item's outline or plate, tests each against the LATER items of the stream (LDS, the same
//                          item for every lane: broadcast reads) and stores its bytes only when none of them covers it.
// So a pixel is written by the last item that covers it and by nobody else, a chroma sample by the owner of its even pixel:
// one writer per byte, whatever the order in which workgroups run.  Byte stores and 64-bit addresses throughout (rgb is three
// bytes a pixel, offsets and pitches may be odd).  Every chunk of a stream builds the same items (a few hundred operations).
#include <stddef.h>

#include "common.h"

// every float64 operation is rounded on its own, like the host code's: no fused multiply-add contraction
#pragma clang fp contract(off)

namespace {

constexpr int MAXB = ME_OVERLAY_MAX_BOXES;
constexpr int MAXI = 2 * MAXB;   // a box and a label per drawn row
constexpr int MAXC = ME_OVERLAY_MAX_CHARS;
constexpr int NGLYPH = ME_OVERLAY_GLYPHS;
constexpr int THREADS = 256;
constexpr int LIM = (1 << 30) + 1024;   // corners are limited to +-LIM: no pixel of a picture of up to 2^30 a side can tell
constexpr int G_DOT = 10, G_HASH = 11, G_M = 12, G_SPACE = 13;
static_assert(MAXB == ME_TRACKS_MAX_DETS && MAXB == 64, "one wave lists the drawn rows; the tracker's detection capacity");

struct Surf {
  unsigned char* base;
  long long bytes, off, h, w, fmt, pitch, uv_off, uv_pitch;
};

// The validity rules of a [n,10] row of me_image_batch_surfaces_u8_f32 (include/millieye_hip.h), in 64 bits and by division.
__host__ __device__ inline bool load_surf(const long long* d, Surf& s) {
  s.base = reinterpret_cast<unsigned char*>(d[0]);
  s.bytes = d[1], s.off = d[2], s.h = d[3], s.w = d[4], s.fmt = d[6], s.pitch = d[7], s.uv_off = d[8], s.uv_pitch = d[9];
  bool valid = d[0] != 0 && s.bytes > 0 && s.h >= 1 && s.w >= 1 && s.h <= (1ll << 30) && s.w <= (1ll << 30);
  long long row = 1;
  if (s.fmt == ME_PIXFMT_RGB || s.fmt == ME_PIXFMT_BGR)
    row = 3 * s.w;
  else if (s.fmt == ME_PIXFMT_NV12)
    row = s.w, valid = valid && (s.h & 1) == 0 && (s.w & 1) == 0;
  else if (s.fmt == ME_PIXFMT_YUYV)
    row = 2 * s.w, valid = valid && (s.w & 1) == 0;
  else
    valid = false;
  valid = valid && s.pitch >= row && row <= s.bytes && s.off >= 0 && s.off <= s.bytes - row;
  valid = valid && s.h - 1 <= (s.bytes - row - s.off) / s.pitch;
  if (valid && s.fmt == ME_PIXFMT_NV12) {
    valid = s.uv_pitch >= s.w && s.uv_off >= 0 && s.uv_off <= s.bytes - s.w;
    valid = valid && s.h / 2 - 1 <= (s.bytes - s.w - s.uv_off) / s.uv_pitch;
  }
  if (s.h == 1) s.pitch = row;   // a pitch nobody steps by may be any number
  if (s.h == 2) s.uv_pitch = s.w;
  return valid;
}

struct Item {
  int x0, y0, x1, y1;       // the covered rectangle, inclusive, not clipped; x0 > x1: no item
  int hx0, hy0, hx1, hy1;   // the hole of an outline; hx0 > hx1 or hy0 > hy1: none
  int slot;                 // a label's row of s_text, -1 for a box
  unsigned char col[3], txt[3];   // the stored bytes of the item's colour and of its glyph pixels
};

__device__ __forceinline__ bool covers(const Item& o, int x, int y) {
  return x >= o.x0 && x <= o.x1 && y >= o.y0 && y <= o.y1 && !(x >= o.hx0 && x <= o.hx1 && y >= o.hy0 && y <= o.hy1);
}

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite64(double v) { return ((unsigned)__double2hiint(v) & 0x7ff00000u) != 0x7ff00000u; }

__device__ __forceinline__ int corner(float v) {
  double r = rint((double)v);
  r = r < -(double)LIM ? -(double)LIM : r > (double)LIM ? (double)LIM : r;
  return (int)r;
}

// decimal digits of v >= 0 into t from position n on; returns the new length
__device__ inline int put_number(unsigned char* t, int n, long long v) {
  unsigned char rev[20];
  int k = 0;
  do {
    rev[k++] = (unsigned char)(v % 10);
    v /= 10;
  } while (v > 0);
  while (k > 0) t[n++] = rev[--k];
  return n;
}

__global__ __launch_bounds__(THREADS) void frame_overlay_kernel(me_frame_overlay_desc d) {
  __shared__ Item s_item[MAXI];
  __shared__ unsigned char s_text[MAXB][MAXC];
  __shared__ unsigned char s_glyph[NGLYPH * 8];
  __shared__ int s_row[MAXB];
  __shared__ int s_drawn;
  __shared__ long long s_before[THREADS], s_total[THREADS];

  const int s = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = d.streams;
  const int32_t* hd = reinterpret_cast<const int32_t*>(d.tail_out);
  const int head = (1 + 2 * S + 3) & ~3;
  const float* table = reinterpret_cast<const float*>(hd + head);

  // ---- the tail's words: this stream's rows start behind the rows of the streams before it (as box_ranges_kernel) -----------
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
  if (tid < NGLYPH * 8) s_glyph[tid] = d.glyphs[tid];
  __syncthreads();
  for (int step = THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      s_before[tid] += s_before[tid + step];
      s_total[tid] += s_total[tid + step];
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  Surf sf;
  const bool surface_ok = load_surf(reinterpret_cast<const long long*>(d.surfaces) + 10 * (size_t)s, sf);
  int status = ME_OVERLAY_OK;
  if (hd[0] != 0 || bad || s_total[0] > d.m) status = ME_OVERLAY_E_INPUT;
  else if (!surface_ok) status = ME_OVERLAY_E_SURFACE;
  if (status != ME_OVERLAY_OK) {   // uniform; no byte of a picture is written
    if (chunk == 0 && tid == 0) d.status[s] = status;
    return;
  }
  const int row0 = (int)s_before[0];   // row0 + kept <= total <= m
  const int kept = hd[1 + S + s];
  const int P = d.palette_len, fmt = (int)sf.fmt;

  // ---- the drawn rows, in order (one wave: ballots) ---------------------------------------------------------------------------
  if (wave == 0) {
    int n = 0;
    for (int base = 0; base < kept && n <= MAXB; base += 64) {
      const int r = base + lane;
      bool draw = false;
      if (r < kept) {
        const float* q = table + (size_t)(row0 + r) * 7;
        const float cls = q[6];
        draw = finite32(q[0]) && finite32(q[1]) && finite32(q[2]) && finite32(q[3]) && finite32(cls) && fabsf(cls) < 2147483648.f;
        if (draw && d.class_count >= 0) {
          const int k = (int)cls;
          bool listed = false;
          for (int c = 0; c < d.class_count; ++c) listed = listed || d.classes[c] == k;
          draw = listed;
        }
      }
      const unsigned long long b = __ballot(draw);
      if (draw) {
        const int pos = n + __popcll(b & ((1ull << lane) - 1ull));
        if (pos < MAXB) s_row[pos] = r;
      }
      n += __popcll(b);
    }
    if (lane == 0) s_drawn = n;
  }
  __syncthreads();
  const int n = s_drawn;
  if (chunk == 0 && tid == 0) d.status[s] = n > MAXB ? ME_OVERLAY_E_BOXES : ME_OVERLAY_OK;
  if (n > MAXB) return;   // uniform

  // ---- one thread per drawn row: its box item and its label item ------------------------------------------------------------------
  if (tid < n) {
    const int r = s_row[tid];
    const float* q = table + (size_t)(row0 + r) * 7;
    const int x1 = corner(q[0]), y1 = corner(q[1]), x2 = corner(q[2]), y2 = corner(q[3]);
    Item box, lab;
    box.x0 = lab.x0 = 1, box.x1 = lab.x1 = 0, box.y0 = lab.y0 = 1, box.y1 = lab.y1 = 0;
    box.hx0 = lab.hx0 = 1, box.hx1 = lab.hx1 = 0, box.hy0 = lab.hy0 = 1, box.hy1 = lab.hy1 = 0;
    box.slot = -1, lab.slot = tid;
    for (int c = 0; c < 3; ++c) box.col[c] = lab.col[c] = box.txt[c] = lab.txt[c] = 0;
    if (x2 >= x1 && y2 >= y1) {
      // the first track row that names this detection
      long long id = -1;
      if (d.tracks) {
        int cnt = d.track_counts[4 * s + 0] == 0 ? d.track_counts[4 * s + 1] : 0;
        cnt = cnt < 0 ? 0 : cnt > ME_TRACKS_MAX_TRACKS ? ME_TRACKS_MAX_TRACKS : cnt;
        const double* tr = d.tracks + (size_t)s * ME_TRACKS_MAX_TRACKS * ME_TRACKS_ROW_COLS;
        for (int t = 0; t < cnt; ++t)
          if (tr[t * ME_TRACKS_ROW_COLS + 9] == (double)r) {
            const double v = tr[t * ME_TRACKS_ROW_COLS];
            if (v >= 0.0 && v <= 2147483647.0) id = (long long)v;
            break;
          }
      }
      const int k = (int)q[6];
      const int idx = ((d.flags & ME_OVERLAY_COLOR_BY_TRACK) && id >= 0) ? (int)(id % P) : ((k % P) + P) % P;
      const unsigned char* rgb = d.palette + (size_t)idx * 3;
      const unsigned char* own = d.palette + ((size_t)fmt * P + idx) * 3;
      const bool dark_text = (299 * (int)rgb[0] + 587 * (int)rgb[1] + 114 * (int)rgb[2]) / 1000 >= 128;
      const bool yuv = fmt == ME_PIXFMT_NV12 || fmt == ME_PIXFMT_YUYV;
      for (int c = 0; c < 3; ++c) {
        box.col[c] = lab.col[c] = own[c];
        lab.txt[c] = yuv ? (c == 0 ? (dark_text ? 16 : 235) : 128) : (dark_text ? 0 : 255);
      }
      const int t = d.thickness;
      box.x0 = x1, box.y0 = y1, box.x1 = x2, box.y1 = y2;
      box.hx0 = x1 + t, box.hy0 = y1 + t, box.hx1 = x2 - t, box.hy1 = y2 - t;
      if (d.flags & ME_OVERLAY_LABELS) {
        unsigned char* text = s_text[tid];
        int len = 0;
        if (id >= 0) {
          text[len++] = G_HASH;
          len = put_number(text, len, id);
          text[len++] = G_SPACE;
        }
        double v = (double)q[4] * 100.0 + 0.5;
        const int conf = v >= 100.0 ? 100 : v >= 0.0 ? (int)floor(v) : 0;   // (a NaN fails both comparisons)
        text[len++] = (unsigned char)(conf / 100);
        text[len++] = G_DOT;
        text[len++] = (unsigned char)(conf / 10 % 10);
        text[len++] = (unsigned char)(conf % 10);
        if (d.ranges && (!d.range_status || d.range_status[s] == 0)) {
          const double rg = d.ranges[(size_t)(row0 + r) * ME_RANGES_ROW_COLS];
          if (finite64(rg)) {
            v = rg * 10.0 + 0.5;
            if (v >= 0.0 && v < 10000.0) {   // 0 <= floor(v) <= 9999
              const int dm = (int)floor(v);
              text[len++] = G_SPACE;
              len = put_number(text, len, dm / 10);
              text[len++] = G_DOT;
              text[len++] = (unsigned char)(dm % 10);
              text[len++] = G_M;
            }
          }
        }
        const int sc = d.font_scale, ph = 8 * sc;   // len <= 12 + 4 + 7 = 23
        const int top = y1 - ph >= 0 ? y1 - ph : y1;
        lab.x0 = x1, lab.y0 = top, lab.x1 = x1 + 6 * sc * len - 1, lab.y1 = top + ph - 1;
      }
    }
    s_item[2 * tid] = box;
    s_item[2 * tid + 1] = lab;
  }
  __syncthreads();

  // ---- paint: the chunks of the stream stride over its items -------------------------------------------------------------------
  const int items = 2 * n;
  const int W = (int)sf.w, H = (int)sf.h;   // <= 2^30
  for (int k = chunk; k < items; k += (int)gridDim.y) {
    const Item it = s_item[k];
    const int cx0 = max(it.x0, 0), cy0 = max(it.y0, 0), cx1 = min(it.x1, W - 1), cy1 = min(it.y1, H - 1);
    if (cx0 > cx1 || cy0 > cy1) continue;   // uniform: no item, or wholly outside
    // the covered pixels as up to four strips of the clipped rectangle: above, below, left of and right of the hole
    const int hx0 = max(it.hx0, cx0), hy0 = max(it.hy0, cy0), hx1 = min(it.hx1, cx1), hy1 = min(it.hy1, cy1);
    int sx[4], sy[4], sw[4], sh[4];
    if (hx0 > hx1 || hy0 > hy1) {
      sx[0] = cx0, sy[0] = cy0, sw[0] = cx1 - cx0 + 1, sh[0] = cy1 - cy0 + 1;
      sw[1] = sw[2] = sw[3] = sh[1] = sh[2] = sh[3] = 0, sx[1] = sx[2] = sx[3] = sy[1] = sy[2] = sy[3] = 0;
    } else {
      sx[0] = cx0, sy[0] = cy0, sw[0] = cx1 - cx0 + 1, sh[0] = hy0 - cy0;
      sx[1] = cx0, sy[1] = hy1 + 1, sw[1] = cx1 - cx0 + 1, sh[1] = cy1 - hy1;
      sx[2] = cx0, sy[2] = hy0, sw[2] = hx0 - cx0, sh[2] = hy1 - hy0 + 1;
      sx[3] = hx1 + 1, sy[3] = hy0, sw[3] = cx1 - hx1, sh[3] = hy1 - hy0 + 1;
    }
    const int cell = 6 * d.font_scale;
    for (int q = 0; q < 4; ++q) {
      const long long count = (long long)sw[q] * sh[q];
      for (long long p = tid; p < count; p += THREADS) {
        int x, y;
        if (count < (1ll << 31)) {
          const unsigned pp = (unsigned)p, ww = (unsigned)sw[q];
          y = sy[q] + (int)(pp / ww), x = sx[q] + (int)(pp % ww);
        } else {
          y = sy[q] + (int)(p / sw[q]), x = sx[q] + (int)(p % sw[q]);
        }
        bool owner = true;
        for (int j = k + 1; j < items && owner; ++j) owner = !covers(s_item[j], x, y);
        if (!owner) continue;
        unsigned char c0 = it.col[0], c1 = it.col[1], c2 = it.col[2];
        if (it.slot >= 0) {   // a plate: is this a glyph pixel?
          const int lx = x - it.x0, ly = y - it.y0;
          const int g = s_text[it.slot][lx / cell], px = (lx % cell) / d.font_scale, py = ly / d.font_scale;
          if (px >= 1 && px <= 5 && py >= 1 && py <= 7 && ((s_glyph[g * 8 + py - 1] >> (5 - px)) & 1))
            c0 = it.txt[0], c1 = it.txt[1], c2 = it.txt[2];
        }
        unsigned char* line = sf.base + sf.off + (long long)y * sf.pitch;
        if (fmt == ME_PIXFMT_RGB || fmt == ME_PIXFMT_BGR) {
          unsigned char* o = line + 3ll * x;
          o[0] = c0, o[1] = c1, o[2] = c2;
        } else if (fmt == ME_PIXFMT_NV12) {
          line[x] = c0;
          if (((x | y) & 1) == 0) {   // the pixel that owns its chroma pair
            unsigned char* o = sf.base + sf.uv_off + (long long)(y >> 1) * sf.uv_pitch + x;
            o[0] = c1, o[1] = c2;
          }
        } else {   // YUYV: Y0 U Y1 V
          line[2ll * x] = c0;
          if ((x & 1) == 0) line[2ll * x + 1] = c1, line[2ll * x + 3] = c2;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int32_t me_frame_overlay_capacity(int32_t which) {
  switch (which) {
    case 0: return MAXB;
    case 1: return MAXC;
    case 2: return NGLYPH;
    case 3: return ME_OVERLAY_MAX_PALETTE;
    case 4: return ME_OVERLAY_MAX_CLASSES;
    default: return -1;
  }
}

int me_frame_overlay_u8(const me_frame_overlay_desc* d, void* stream) {
  ME_REQUIRE(d, ME_E_NULLPTR, "me_frame_overlay_u8: null descriptor");
  ME_REQUIRE(d->tail_out && d->surfaces && d->surfaces_host && d->palette && d->glyphs && d->status, ME_E_NULLPTR,
             "me_frame_overlay_u8: null pointer");
  ME_REQUIRE((d->tracks != nullptr) == (d->track_counts != nullptr), ME_E_NULLPTR,
             "me_frame_overlay_u8: tracks and track_counts go together");
  ME_REQUIRE(d->ranges || !d->range_status, ME_E_NULLPTR, "me_frame_overlay_u8: range_status without ranges");
  ME_REQUIRE(d->streams > 0 && d->streams <= 65535 && d->m >= 0 && d->m <= 32768, ME_E_BADARG,
             "me_frame_overlay_u8: %d streams, m = %d", d->streams, d->m);
  ME_REQUIRE(d->thickness >= 1 && d->thickness <= 8 && d->font_scale >= 1 && d->font_scale <= 4, ME_E_BADARG,
             "me_frame_overlay_u8: thickness %d (1 .. 8), font_scale %d (1 .. 4)", d->thickness, d->font_scale);
  ME_REQUIRE(d->palette_len >= 1 && d->palette_len <= ME_OVERLAY_MAX_PALETTE, ME_E_BADARG,
             "me_frame_overlay_u8: palette_len %d (1 .. %d)", d->palette_len, ME_OVERLAY_MAX_PALETTE);
  ME_REQUIRE(d->class_count >= -1 && d->class_count <= ME_OVERLAY_MAX_CLASSES && (d->class_count <= 0 || d->classes), ME_E_BADARG,
             "me_frame_overlay_u8: class_count %d (-1 .. %d, with a list)", d->class_count, ME_OVERLAY_MAX_CLASSES);
  ME_REQUIRE((d->flags & ~(ME_OVERLAY_LABELS | ME_OVERLAY_COLOR_BY_TRACK)) == 0, ME_E_BADARG,
             "me_frame_overlay_u8: unknown flags 0x%x", d->flags);
  ME_REQUIRE(me::aligned16(d->tail_out), ME_E_ALIGN, "me_frame_overlay_u8: tail_out not 16-byte aligned");
  // refuse, do not clamp: every row of the descriptor's host copy keeps the rules of me_image_batch_surfaces_u8_f32
  for (int s = 0; s < d->streams; ++s) {
    Surf sf;
    const long long* row = reinterpret_cast<const long long*>(d->surfaces_host) + 10 * (size_t)s;
    ME_REQUIRE(load_surf(row, sf), ME_E_BADARG,
               "me_frame_overlay_u8: surface %d is invalid (bytes %lld, off %lld, h %lld, w %lld, fmt %lld, pitch %lld, uv_off "
               "%lld, uv_pitch %lld)", s, row[1], row[2], row[3], row[4], row[6], row[7], row[8], row[9]);
  }
  // chunks per stream: the items of a stream (128 at most) are dealt out to this many workgroups
  const unsigned chunks = d->streams <= 64 ? 8 : d->streams <= 1024 ? 4 : 1;
  hipLaunchKernelGGL(frame_overlay_kernel, dim3(d->streams, chunks), dim3(THREADS), 0, (hipStream_t)stream, *d);
  return me::check_launch("frame_overlay_kernel");
}

}  // extern "C"
