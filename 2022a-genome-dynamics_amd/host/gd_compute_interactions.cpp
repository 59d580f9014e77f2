// gd_compute_interactions -- the reference's compute_interactions (2-signal/src/compute_interactions): the local decay signals D1.. and the insulation
// ratios I1.. of every bin of a cooler's resolution, the table model_genome classifies A/B/u beads from.
// The command line, the reads and the outputs are in gd_hic_cli.hpp; the sums and signals are libgdyn's (include/gdyn_hic.h).
#include "gd_hic_cli.hpp"

int main(int argc, char **argv) { return gd::hic::main(gd::hic::program::interactions, argc, argv); }
