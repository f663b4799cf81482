// Host-only sweep of the two route functions of include/geoa3_hip_debug.h over every cloud size, for a sanitizer build of the
// host code of geom_reg.hip and geom_uniform.hip (no GPU work: neither function launches anything):
//   hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -Xarch_host -fsanitize=address,undefined \
//         tools/route_sweep.cpp geoa3_amd/csrc/geom_reg.hip geoa3_amd/csrc/geom_uniform.hip \
//         -Lgeoa3_amd/lib -lgeoa3_hip -Wl,-rpath,$PWD/geoa3_amd/lib -o route_sweep && ./route_sweep
// (the two files' own definitions take precedence over the library's, which serves the symbols they call)
#include <cstdio>
#include "../include/geoa3_hip_debug.h"

int main() {
  const double one[1] = {0.004}, five[5] = {0.004, 0.006, 0.008, 0.010, 0.012}, eight[8] = {0.004, 0.006, 0.008, 0.010,
                                                                                             0.012, 0.014, 0.016, 0.018};
  long counts[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int N = 1; N <= 8200; ++N) {
    for (int mode = -1; mode <= 4; ++mode)
      for (int k : {0, 1, 4, 16, 63, 64}) {
        const int r = geoa3_debug_reg_route(mode, N, k);
        if (r < 0 || r > GEOA3_REG_ROUTE_REFUSED) return 1;
        ++counts[0][r];
      }
    for (int k : {0, 1, 2, 8, 9}) {
      const int rs[4] = {geoa3_debug_uniform_route(2, N, one, 1, 1.0, k), geoa3_debug_uniform_route(250, N, five, 5, 1.0, k),
                         geoa3_debug_uniform_route(1, N, eight, 8, 0.5, k), geoa3_debug_uniform_route(2, N, nullptr, 1, 1.0, k)};
      for (int r : rs) {
        if (r > GEOA3_UNIFORM_ROUTE_WORKSPACE || r < GEOA3_ENOSUPPORT) return 1;
        ++counts[1][r < 0 ? 2 : r];
      }
    }
  }
  std::printf("reg: LDS %ld WORKSPACE %ld REFUSED %ld; uniform: LDS %ld WORKSPACE %ld refused %ld\n", counts[0][0], counts[0][1],
              counts[0][2], counts[1][0], counts[1][1], counts[1][2]);
  return 0;
}
