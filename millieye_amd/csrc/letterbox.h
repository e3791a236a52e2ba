// The letterbox geometry of the rectangular input path, shared by csrc/input.hip (frames, heat maps) and csrc/radar.hip (the
// network's radar boxes); utils.utils.letterbox_geometry is the same rule on the host.
// Canvas H x W, a = H / gcd(H, W), b = W / gcd(H, W).  A picture h x w is padded with zeros to the smallest rectangle of the
// canvas's aspect ratio that holds it: k = max(ceil(h / a), ceil(w / b)), Ph = a k, Pw = b k (so Ph / H == Pw / W exactly);
// top = (Ph - h) / 2 and left = (Pw - w) / 2 rounded down, the rest of the padding goes behind.  H == W: pad_to_square.
#pragma once

namespace me {

inline int gcd_i32(int x, int y) {
  while (y) {
    const int t = x % y;
    x = y;
    y = t;
  }
  return x;
}

}  // namespace me

struct LetterboxGeom {
  int Ph, Pw, top, left;
  bool ok;   // Ph and Pw within 2^30 (otherwise every field is a harmless 1 / 0)
};

// h, w in [1, 2^30], a, b in [1, 2^30): k is computed in 64 bits
__device__ inline LetterboxGeom letterbox_geom(int h, int w, int a, int b) {
  const long long kh = ((long long)h + a - 1) / a, kw = ((long long)w + b - 1) / b;
  const long long k = kh > kw ? kh : kw, Ph = a * k, Pw = b * k;
  LetterboxGeom g;
  g.ok = Ph <= (1ll << 30) && Pw <= (1ll << 30);
  g.Ph = g.ok ? (int)Ph : 1;
  g.Pw = g.ok ? (int)Pw : 1;
  g.top = g.ok ? (g.Ph - h) / 2 : 0;
  g.left = g.ok ? (g.Pw - w) / 2 : 0;
  return g;
}
