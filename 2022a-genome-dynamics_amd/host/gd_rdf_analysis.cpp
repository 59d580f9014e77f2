// gd_rdf_analysis -- rdf_analysis of the reference (4-sim-ab/box/src/rdf_analysis) on the device: the radial distribution of
// the selected beads (--type A: A factor 1, --type B: A factor 0, otherwise every bead) around themselves in every snapshot of
// a stage-4 box trajectory, one tab-separated line of n_bins values per frame on stdout.
//   gd_rdf_analysis [--type T] [--steps RANGE] [--bin-width W] [--max-distance R] [--dry-run] FILE
#include "gd_rdf_cli.hpp"

int main(int argc, char **argv) { return gd::rdf::main(argc, argv, false); }
