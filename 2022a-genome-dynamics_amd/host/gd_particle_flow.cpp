// gd_particle_flow -- analyze_particle_flow of the reference (5-sim-genome/src/analyze_particle_flow) on the device:
// for every trajectory file, the mean velocity of the beads within --scan-radius of each bead in every interphase frame,
// written to /particle_flow/<name>/<sample>/{position,velocity} of the output file.
//   gd_particle_flow [--name N] [--smoothing W] [--velocity-delay D] --scan-radius R [--jobs J] [--dry-run] outfile trajfiles...
#include "gd_flow_cli.hpp"

int main(int argc, char **argv)
{
    using namespace gd::flow;
    return gd::flow::main(argc, argv, false, [](options const &o, std::string const &config, std::string const &name, char const *prog) {
        device dev;
        open(dev);
        particle_writer out(o.outfile, name, config);
        bool const smooth = smoothed(o);
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = load_history(path, F, N);
            sw.read += sw.lap();
            std::vector<double> pos(smooth ? (std::size_t)F * N * 3 : 0);
            std::vector<float> flows((std::size_t)F * N * 3);
            gd::cli::check(gd_flow_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_flow_velocities(dev.h, smooth ? (uint32_t)o.smoothing : 0, (uint32_t)o.delay, smooth ? pos.data() : nullptr, nullptr));
            gd::cli::check(gd_flow_particle(dev.h, o.radius, flows.data()));
            sw.compute += sw.lap();
            out.put(gd::cli::sample_name(path), F, N, hist.data(), smooth ? pos.data() : nullptr, flows.data());
            sw.write += sw.lap();
        }
        out.finish();
        sw.write += sw.lap();
        sw.report(prog);
    });
}
