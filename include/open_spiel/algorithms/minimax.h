// forwards to the MI355X host mirror: see include/open_spiel/spiel.h
// algorithms::AlphaBetaSearch (minimax.h:25-50) is the mirror's: a device search of the root, or the host recursion
// where a value_function is given (open_spiel_amd/csrc/host/osg_spiel.h).  ExpectiminimaxSearch is not declared: no
// game of the path is both perfect-information and stochastic.
#include "open_spiel/spiel.h"
