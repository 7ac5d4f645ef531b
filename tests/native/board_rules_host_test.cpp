// Host-side run of the board rules of open_spiel_amd/csrc/osg_game_boards.h (C4T / HexT: what every batch kernel maps
// over its states) on given action histories, for ANY game string parse_game accepts — the run-time geometry paths in
// particular, whose shift amounts come from the parameters.  The rules are device functions in the library; this program
// compiles them for the host by redefining the marker macro before the headers that use it, and takes the parser
// (osg_game_spec.hip) into the same translation unit, so the Params are the ones a device batch would get.
//   hipcc --cuda-host-only -x hip -O1 -fsanitize=address,undefined -I open_spiel_amd/csrc tests/native/board_rules_host_test.cpp
// Usage: board_rules_host_test GAME_STRING STRIDE < histories      (one history per line: action ids, blank-separated)
// Prints per history and ply t = 0 .. len one line
//   t mask-words(hex, ':'-joined) current_player terminal returns0 returns1 [fused: illegal terminal outcome open-columns]
// (the bracketed part for connect_four: C4T::fused_step of the action taken from t - 1, on a copy), and at every
// STRIDE-th ply and the last one line "obs P hexdigits" per player: the observation tensor's entries (0 / 1) packed four
// to a digit, read through ObsCursor, after checking that obs_at gives the same entries.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "osg_common.h"
#undef OSG_D
#define OSG_D __host__ __device__ __forceinline__
#include "osg_game_spec.hip"

using namespace osg;

static bool p_plain(const C4Params&) { return false; }
template <int NW> static bool p_plain(const HexParamsT<NW>& p) { return p.plain_obs != 0; }

template <class G>
static int print_obs(const typename G::Params& p, const typename G::State& s, int size) {
  for (int player = 0; player < 2; ++player) {
    typename G::ObsCursor cur;
    std::string digits;
    int acc = 0;
    // the device's tensor kernel starts a cursor per chunk and (hex) never lets one cross a plane: restart per plane
    const int planes = is_hex<G>::value && !p_plain(p) ? 9 : 1, per = size / planes;
    for (int idx = 0; idx < size; ++idx) {
      if (idx % per == 0) cur.init(p, s, player, 0, idx);
      const float a = cur.next(p, s, player, 0), b = G::obs_at(p, s, player, 0, idx);
      if (a != b || (a != 0.0f && a != 1.0f)) {
        printf("FAILED: cursor %g, obs_at %g at entry %d\n", a, b, idx);
        return 1;
      }
      acc |= (a != 0.0f ? 1 : 0) << (idx & 3);
      if ((idx & 3) == 3 || idx == size - 1) {
        digits += "0123456789abcdef"[acc];
        acc = 0;
      }
    }
    printf("obs %d %s\n", player, digits.c_str());
  }
  return 0;
}

template <class G>
static int run(const typename G::Params& p, const osg_game_desc& d, int stride) {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<int> hist;
    for (int a; in >> a;) hist.push_back(a);
    typename G::State s = G::initial(p);
    const int len = static_cast<int>(hist.size());
    printf("history %d\n", len);
    std::string fused;
    for (int t = 0; t <= len; ++t) {
      const auto m = G::legal(p, s);
      printf("%d ", t);
      for (int w = 0; w < d.mask_words; ++w) printf("%s%08x", w ? ":" : "", m.w[w]);
      double r[kMaxPlayers];
      G::returns(p, s, r);
      printf(" %d %d %g %g%s\n", G::current_player(p, s), G::terminal(p, s) ? 1 : 0, r[0], r[1], fused.c_str());
      if (t % stride == 0 || t == len)
        if (print_obs<G>(p, s, d.obs_size)) return 1;
      if (t == len) break;
      const int a = hist[t];
      if (a < 0 || a >= 32 * static_cast<int>(sizeof(m.w) / sizeof(m.w[0])) || !m.test(a)) {
        printf("FAILED: action %d is not legal at ply %d\n", a, t);
        return 1;
      }
      fused.clear();
      if constexpr (!is_hex<G>::value) {
        typename G::State c = s;
        bool illegal = false, term = false;
        int outcome = 0;
        const uint32_t open = G::fused_step(p, c, a, illegal, term, outcome);
        char buf[64];
        snprintf(buf, sizeof buf, " fused %d %d %d %08x", illegal ? 1 : 0, term ? 1 : 0, outcome, open);
        fused = buf;
        typename G::State viaapply = s;
        G::apply(p, viaapply, a);
        if (c.x != viaapply.x || c.o != viaapply.o) {
          printf("FAILED: fused_step and apply leave different boards at ply %d\n", t);
          return 1;
        }
      }
      G::apply(p, s, a);
    }
  }
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  GameSpec spec;
  if (parse_game(argv[1], &spec) != OSG_OK) {
    printf("REFUSED: %s\n", osg_last_error());
    return 3;
  }
  const int stride = atoi(argv[2]);
  return for_game(spec, [&](auto tag, const auto& p) {
    using G = typename decltype(tag)::type;
    if constexpr (std::is_same<G, C4>::value || std::is_same<G, C4Wide>::value || std::is_same<G, C4Std>::value || is_hex<G>::value)
      return run<G>(p, spec.desc, stride < 1 ? 1 : stride);
    else
      return 2;
  });
}
