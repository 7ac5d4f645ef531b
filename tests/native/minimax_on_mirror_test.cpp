// algorithms::AlphaBetaSearch through the drop-in header include/open_spiel/algorithms/minimax.h, with the reference's
// signature: the three tic_tac_toe cases of the reference's minimax_test.cc as it states them (no value function,
// depth_limit -1, kInvalidPlayer), one call with a host value_function at depth 1, the fatal error at a depth limit with
// no value function, and the node budget (the mirror's extra trailing parameter).
#include <iostream>
#include <memory>
#include <string>
#include <utility>

#include "open_spiel/algorithms/minimax.h"
#include "open_spiel/spiel.h"
#include "open_spiel/spiel_utils.h"

namespace open_spiel {
namespace algorithms {
namespace {

void AlphaBetaSearchTest_TicTacToe() {
  std::shared_ptr<const Game> game = LoadGame("tic_tac_toe");
  std::pair<double, Action> value_and_action = AlphaBetaSearch(*game, nullptr, {}, -1, kInvalidPlayer);
  SPIEL_CHECK_EQ(0.0, value_and_action.first);
  SPIEL_CHECK_EQ(0, value_and_action.second);
}

void AlphaBetaSearchTest_TicTacToe_Win() {
  std::shared_ptr<const Game> game = LoadGame("tic_tac_toe");
  std::unique_ptr<State> state = game->NewInitialState();
  state->ApplyAction(4);
  state->ApplyAction(1);
  std::pair<double, Action> value_and_action = AlphaBetaSearch(*game, state.get(), {}, -1, kInvalidPlayer);
  SPIEL_CHECK_EQ(1.0, value_and_action.first);
  SPIEL_CHECK_EQ(0, value_and_action.second);
  SPIEL_CHECK_EQ(2, static_cast<int>(state->History().size()));   // the caller's state is left as it was
}

void AlphaBetaSearchTest_TicTacToe_Loss() {
  std::shared_ptr<const Game> game = LoadGame("tic_tac_toe");
  std::unique_ptr<State> state = game->NewInitialState();
  state->ApplyAction(5);
  state->ApplyAction(4);
  state->ApplyAction(3);
  state->ApplyAction(8);
  std::pair<double, Action> value_and_action = AlphaBetaSearch(*game, state.get(), {}, -1, kInvalidPlayer);
  SPIEL_CHECK_EQ(-1.0, value_and_action.first);
}

// value_function = a constant at depth 1: the host recursion; every child is worth 0.25, the first one is kept.
void AlphaBetaSearchTest_HostValueFunction() {
  std::shared_ptr<const Game> game = LoadGame("tic_tac_toe");
  int calls = 0;
  std::pair<double, Action> value_and_action =
      AlphaBetaSearch(*game, nullptr, [&calls](const State&) { ++calls; return 0.25; }, 1, kInvalidPlayer);
  SPIEL_CHECK_EQ(0.25, value_and_action.first);
  SPIEL_CHECK_EQ(0, value_and_action.second);
  SPIEL_CHECK_EQ(9, calls);
  calls = 0;
  value_and_action = AlphaBetaSearch(*game, nullptr, [&calls](const State&) { ++calls; return 0.25; }, 1, kInvalidPlayer,
                                     /*use_undo=*/false);
  SPIEL_CHECK_EQ(0.25, value_and_action.first);
  SPIEL_CHECK_EQ(9, calls);
}

}  // namespace
}  // namespace algorithms
}  // namespace open_spiel

int main() {
  using namespace open_spiel;
  algorithms::AlphaBetaSearchTest_TicTacToe();
  algorithms::AlphaBetaSearchTest_TicTacToe_Win();
  algorithms::AlphaBetaSearchTest_TicTacToe_Loss();
  algorithms::AlphaBetaSearchTest_HostValueFunction();
  // the mirror's errors are exceptions (SpielFatalError throws SpielException)
  std::shared_ptr<const Game> game = LoadGame("tic_tac_toe");
  bool thrown = false;
  try {
    algorithms::AlphaBetaSearch(*game, nullptr, {}, 3, kInvalidPlayer);
  } catch (const SpielException& e) {
    thrown = std::string(e.what()).find("We assume we can walk the full depth of the tree.") != std::string::npos;
  }
  SPIEL_CHECK_TRUE(thrown);
  SPIEL_CHECK_EQ(0.0, algorithms::AlphaBetaSearch(*game, nullptr, {}, -1, kInvalidPlayer, true, 18297).first);
  thrown = false;
  try {
    algorithms::AlphaBetaSearch(*game, nullptr, {}, -1, kInvalidPlayer, true, 18296);
  } catch (const SpielException& e) {
    thrown = std::string(e.what()).find("node budget of 18296") != std::string::npos;
  }
  SPIEL_CHECK_TRUE(thrown);
  thrown = false;
  try {
    algorithms::AlphaBetaSearch(*LoadGame("kuhn_poker"), nullptr, {}, -1, kInvalidPlayer);
  } catch (const SpielException&) {
    thrown = true;
  }
  SPIEL_CHECK_TRUE(thrown);
  std::cout << "minimax_on_mirror_test: ok" << std::endl;
  return 0;
}
