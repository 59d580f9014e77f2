// gd_rdf_analysis_hetero -- rdf_analysis_hetero of the reference (4-sim-ab/box/src/rdf_analysis_hetero) on the device: the
// radial distribution of the other beads around the centres of one type (--type A, the default, or B) in every snapshot,
// one tab-separated line of n_bins values per frame on stdout.
//   gd_rdf_analysis_hetero [--type T] [--bin-width W] [--max-distance R] [--dry-run] FILE
#include "gd_rdf_cli.hpp"

int main(int argc, char **argv) { return gd::rdf::main(argc, argv, true); }
