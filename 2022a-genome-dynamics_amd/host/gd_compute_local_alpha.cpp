// gd_compute_local_alpha -- the reference's compute_local_alpha (2-signal/src/compute_local_alpha): the local contact-decay exponent of every bin of a
// cooler's resolution.
// The command line, the reads and the outputs are in gd_hic_cli.hpp; the sums and signals are libgdyn's (include/gdyn_hic.h).
#include "gd_hic_cli.hpp"

int main(int argc, char **argv) { return gd::hic::main(gd::hic::program::alpha, argc, argv); }
