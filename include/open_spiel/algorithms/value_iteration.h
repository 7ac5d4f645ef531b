// forwards to the MI355X host mirror: see include/open_spiel/spiel.h
// algorithms::ValueIteration (value_iteration.h:41-42) is the mirror's: one device enumeration and backward sweep
// (open_spiel_amd/csrc/host/osg_spiel.h) for tic_tac_toe, connect_four and hex without the swap move.
#include "open_spiel/spiel.h"
