// gd_hic_power_law -- the reference's hic_power_law (5-sim-genome/scripts/hic_power_law): the mean cis contact against genomic distance of a cooler's
// resolution, the experimental P(s).
// The command line, the reads and the outputs are in gd_hic_cli.hpp; the sums and signals are libgdyn's (include/gdyn_hic.h).
#include "gd_hic_cli.hpp"

int main(int argc, char **argv) { return gd::hic::main(gd::hic::program::power_law, argc, argv); }
