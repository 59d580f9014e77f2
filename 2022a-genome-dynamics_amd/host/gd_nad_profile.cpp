// gd_nad_profile -- the reference's nad_profile (5-sim-genome/src/nad_profile): the summed nucleolus-contact profile of the chosen chromosomes.
// The command line, the reads and the outputs are in gd_cmap_cli.hpp; the sums are libgdyn's (include/gdyn_cmap.h).
#include "gd_cmap_cli.hpp"

int main(int argc, char **argv) { return gd::cmap::main(gd::cmap::program::nad_profile, argc, argv); }
