// gd_analyze_lamina -- analyze_lamina of the reference (5-sim-genome/src/analyze_lamina) on the device:
//   gd_analyze_lamina distance [--dry-run] outfile trajfiles...
//        for every trajectory file, the distance of every bead from the nuclear wall in every interphase frame, written to
//        /distance/<file name> of the output file (float32; shuffle, scale-offset D-scale 3, deflate 1), and the metadata of
//        the first trajectory to /metadata/{simulation_config, particle_types, chromosome_ranges, chromosome_names}
//   gd_analyze_lamina contact [--name uniform] --contact-distance D [--dry-run] outfile
//        for every /distance/<key> of the output file as stored, distance < D to /contact/<name>/<key> and the mean over the
//        keys to /average_contact/<name>
#include "gd_lamina_cli.hpp"

int main(int argc, char **argv) { return gd::lamina::main(argc, argv); }
