// gd_gw_contact_matrix -- the reference's gw_contact_matrix (5-sim-genome/src/gw_contact_matrix): the genome-wide rebinned contact matrix as HDF5.
// The command line, the reads and the outputs are in gd_cmap_cli.hpp; the sums are libgdyn's (include/gdyn_cmap.h).
#include "gd_cmap_cli.hpp"

int main(int argc, char **argv) { return gd::cmap::main(gd::cmap::program::gw_contact_matrix, argc, argv); }
