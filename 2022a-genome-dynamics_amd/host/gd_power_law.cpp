// gd_power_law -- the reference's power_law (5-sim-genome/src/power_law): the three contact-probability exponents of each trajectory.
// The command line, the reads and the outputs are in gd_cmap_cli.hpp; the sums are libgdyn's (include/gdyn_cmap.h).
#include "gd_cmap_cli.hpp"

int main(int argc, char **argv) { return gd::cmap::main(gd::cmap::program::power_law, argc, argv); }
