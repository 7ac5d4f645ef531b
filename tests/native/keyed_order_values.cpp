// Values of the keyed orders of open_spiel_amd/csrc/osg_common.h (order_base, order_key, fill_base, fill_key and the
// root path hash) for a fixed list of inputs, one line each: tests/test_sampling_stats_cpu.py compares the NumPy
// restatements of tests/sampling_stats.py with them, so that the statistical tests of the restatement speak about
// the functions the kernels run.
//   hipcc --cuda-host-only -x hip -O2 -I open_spiel_amd/csrc tests/native/keyed_order_values.cpp
#include <cstdio>
#include <cstdint>
#include "osg_common.h"

int main() {
  const uint64_t seeds[] = {0ULL, 0x5A3D1EULL, 0xFFFFFFFFFFFFFFFFULL, 0x0123456789ABCDEFULL};
  const uint64_t roots[] = {0ULL, 1ULL, 12345ULL, (1ULL << 33) + 7ULL, (1ULL << 63) + 5ULL};
  const uint64_t subs[] = {0ULL, 1ULL, 1023ULL, (1ULL << 32) + 3ULL, (1ULL << 40) + 9ULL};
  const int ids[] = {0, 1, 8, 80, 127, 255, 256, 360};
  printf("path_hash_root %llu\n", static_cast<unsigned long long>(osg::path_hash_root()));
  for (uint64_t seed : seeds)
    for (uint64_t root : roots) {
      const uint64_t ob = osg::order_base(seed, root);
      printf("order_base %llu %llu %llu\n", (unsigned long long)seed, (unsigned long long)root, (unsigned long long)ob);
      for (int a : ids)
        printf("order_key %llu %llu %d %u\n", (unsigned long long)seed, (unsigned long long)root, a,
               osg::order_key(ob, osg::path_hash_root(), a));
      for (uint64_t sub : subs) {
        const uint64_t fb = osg::fill_base(seed, root, sub);
        printf("fill_base %llu %llu %llu %llu\n", (unsigned long long)seed, (unsigned long long)root,
               (unsigned long long)sub, (unsigned long long)fb);
        for (int c : ids)
          printf("fill_key %llu %llu %llu %d %llu\n", (unsigned long long)seed, (unsigned long long)root,
                 (unsigned long long)sub, c, (unsigned long long)osg::fill_key(fb, c));
      }
    }
  return 0;
}
