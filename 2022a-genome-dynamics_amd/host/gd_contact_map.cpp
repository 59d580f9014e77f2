// gd_contact_map -- the reference's contact_map (5-sim-genome/src/contact_map): the summed Hi-C-like matrix of the chosen chromosomes as TSV.
// The command line, the reads and the outputs are in gd_cmap_cli.hpp; the sums are libgdyn's (include/gdyn_cmap.h).
#include "gd_cmap_cli.hpp"

int main(int argc, char **argv) { return gd::cmap::main(gd::cmap::program::contact_map, argc, argv); }
