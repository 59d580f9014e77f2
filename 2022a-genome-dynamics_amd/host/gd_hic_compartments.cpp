// gd_hic_compartments -- the compartment analysis of the reference's hic_analysis/cool.py (2-signal/src and 5-sim-genome/src) as a
// program: dense cis contact matrices of a cooler's resolution, observed / expected by the mean contact per distance, and the leading
// principal components of every requested chromosome (the first is the A/B compartment signal).  The reference has no command for it.
// The command line, the reads and the outputs are in gd_hic_cli.hpp; the matrices and the solver are libgdyn's (include/gdyn_hic.h).
#include "gd_hic_cli.hpp"

int main(int argc, char **argv) { return gd::hic::main(gd::hic::program::compartments, argc, argv); }
