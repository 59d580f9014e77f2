// gd_downsample -- the reference's downsample (2-signal/src/downsample): a signal table at a coarser resolution, boxcar means per chromosome.
// Host only: no device work.
// The command line, the reads and the outputs are in gd_hic_cli.hpp; the sums and signals are libgdyn's (include/gdyn_hic.h).
#include "gd_hic_cli.hpp"

int main(int argc, char **argv) { return gd::hic::main(gd::hic::program::downsample, argc, argv); }
