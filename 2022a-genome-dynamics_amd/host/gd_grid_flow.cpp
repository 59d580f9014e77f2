// gd_grid_flow -- analyze_grid_flow of the reference (5-sim-genome/src/analyze_grid_flow) on the device: for every
// trajectory file, the mean velocity of the beads within --scan-radius of each point of a regular grid and their number,
// written to /grid_flow/<name>/<sample>/{flows,coverages} of the output file, with the grid under .grid/.
//   gd_grid_flow [--name N] [--smoothing W] [--velocity-delay D] --scan-radius R --grid-interval H --x-range A,B --y-range A,B
//                --z-range A,B [--jobs J] [--dry-run] outfile trajfiles...
#include "gd_flow_cli.hpp"

int main(int argc, char **argv)
{
    using namespace gd::flow;
    return gd::flow::main(argc, argv, true, [](options const &o, std::string const &config, std::string const &name, char const *prog) {
        mesh const m(o);
        device dev;
        open(dev);
        grid_writer out(o.outfile, name, config, m);
        bool const smooth = smoothed(o);
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = load_history(path, F, N);
            sw.read += sw.lap();
            std::vector<float> flows((std::size_t)F * m.G * 3);
            std::vector<int32_t> cov((std::size_t)F * m.G);
            gd::cli::check(gd_flow_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_flow_velocities(dev.h, smooth ? (uint32_t)o.smoothing : 0, (uint32_t)o.delay, nullptr, nullptr));
            gd::cli::check(gd_flow_grid(dev.h, o.radius, m.points.data(), (uint32_t)m.G, flows.data(), cov.data()));
            int const factor = scaleoffset_factor(flows);
            sw.compute += sw.lap();
            out.put(gd::cli::sample_name(path), F, flows, cov, factor);
            sw.write += sw.lap();
        }
        out.finish();
        sw.write += sw.lap();
        sw.report(prog);
    });
}
