// Stand-alone host check of weightmap.hip's window scan (two_nearest, a __host__ __device__ function) against a
// brute-force per-id minimum over the window, on random scenes at R = 1..48; no GPU is touched.  From the
// repository root, with the host code under AddressSanitizer and UBSan:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip tools/weightmap_scan_check.cpp \
//     enhanced-unet_amd/csrc/capi.hip -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//     -o weightmap_scan_check && ./weightmap_scan_check
// Exit status 0 and "bad 0" mean every pixel agreed.
#include "../enhanced-unet_amd/csrc/weightmap.hip"
#include <map>
#include <random>
#include <algorithm>

int main() {
  std::mt19937 rng(1);
  long checked = 0, bad = 0;
  for (int trial = 0; trial < 600; ++trial) {
    const int R = 1 + rng() % 48;
    const int H = 1 + rng() % WT, W = 1 + rng() % WT;  // the part of one tile that lies inside the image
    const int SW = WT + 2 * R, SH = SW;                // the kernel's staged region: square, <= 128 wide
    std::vector<uint32_t> st((size_t)SW * SH, 0u);
    const int nb = rng() % 7;
    const uint32_t ids[5] = {3u, 70000u, 7u, 0xFFFFFFFFu, 12u};
    for (int b = 0; b < nb; ++b) {  // discs anywhere in the staged region: the halo holds cells too
      const int cy = rng() % SH, cx = rng() % SW, r = rng() % 9;
      const uint32_t id = ids[rng() % 5];
      for (int y = std::max(0, cy - r); y <= std::min(SH - 1, cy + r); ++y)
        for (int x = std::max(0, cx - r); x <= std::min(SW - 1, cx + r); ++x)
          if ((y - cy) * (y - cy) + (x - cx) * (x - cx) <= r * r) st[(size_t)y * SW + x] = id;
    }
    std::vector<uint32_t> occ((size_t)SH * MW, 0u);  // the candidate masks, built as the kernel builds them
    for (int sy = 0; sy < SH; ++sy)
      for (int sx = 0; sx < SW; ++sx)
        if (candidate(st.data(), SW, sx, sy)) occ[(size_t)sy * MW + (sx >> 5)] |= 1u << (sx & 31);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        if (st[(size_t)(y + R) * SW + x + R]) continue;
        const Near2 nn = two_nearest(st.data(), occ.data(), SW, x + R, y + R, R);
        std::map<uint32_t, unsigned> best;
        for (int dy = -R; dy <= R; ++dy)
          for (int dx = -R; dx <= R; ++dx) {
            const uint32_t id = st[(size_t)(y + R + dy) * SW + x + R + dx];
            if (!id) continue;
            const unsigned d = dy * dy + dx * dx;
            auto it = best.find(id);
            if (it == best.end() || d < it->second) best[id] = d;
          }
        std::vector<unsigned> v;
        for (auto& kv : best) v.push_back(kv.second);
        std::sort(v.begin(), v.end());
        const unsigned e1 = v.size() > 0 ? v[0] : NONE, e2 = v.size() > 1 ? v[1] : NONE;
        ++checked;
        if (nn.d1 != e1 || nn.d2 != e2) {
          if (bad++ < 10) printf("trial %d R %d (%d,%d): got %u %u want %u %u\n", trial, R, x, y, nn.d1, nn.d2, e1, e2);
        }
      }
  }
  printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
