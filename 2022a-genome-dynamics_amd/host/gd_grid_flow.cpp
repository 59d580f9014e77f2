// gd_grid_flow -- analyze_grid_flow of the reference (5-sim-genome/src/analyze_grid_flow) on the device: for every
// trajectory file, the mean velocity of the beads within --scan-radius of each point of a regular grid and their number,
// written to /grid_flow/<name>/<sample>/{flows,coverages} of the output file, with the grid under .grid/.
//   gd_grid_flow [--name N] [--smoothing W] [--velocity-delay D] --scan-radius R --grid-interval H --x-range A,B --y-range A,B
//                --z-range A,B [--jobs J] [--dry-run] outfile trajfiles...
#include "gd_flow_cli.hpp"

namespace {

std::vector<double> arange(double start, double stop, double step)      // numpy.arange for floats, its fill rule included
{
    double const len = std::ceil((stop - start) / step);
    std::vector<double> out(len > 0 ? (std::size_t)len : 0);
    if (out.empty()) return out;
    out[0] = start;
    if (out.size() > 1) out[1] = start + step;
    double const delta = (start + step) - start;
    for (std::size_t i = 2; i < out.size(); i++) out[i] = start + (double)i * delta;
    return out;
}

// estimate_scaleoffset_factor(values, q=1): -floor(log10(0.1 * percentile(values[values > 0], 1))) in float32, numpy's linear rule
int scaleoffset_factor(std::vector<float> const &v)
{
    std::vector<float> pos;
    for (float x : v) if (x > 0) pos.push_back(x);
    if (pos.empty()) throw std::runtime_error("no positive flow component: the scale-offset factor is undefined");
    std::sort(pos.begin(), pos.end());
    double const idx = 0.01 * (double)(pos.size() - 1);
    std::size_t const lo = (std::size_t)std::floor(idx);
    std::size_t const hi = std::min(lo + 1, pos.size() - 1);
    float const t = (float)(idx - (double)lo), a = pos[lo], b = pos[hi], diff = b - a;
    float const p = t >= 0.5f ? b - diff * (1.0f - t) : a + diff * t;
    float const resolution = 0.1f * p;
    return -(int)std::floor(std::log10(resolution));
}

std::vector<std::string> remove_duplicates(std::vector<std::string> const &xs)      // keeps the last occurrence
{
    std::vector<std::string> out;
    for (std::size_t i = 0; i < xs.size(); i++)
        if (std::find(xs.begin() + (long)i + 1, xs.end(), xs[i]) == xs.end()) out.push_back(xs[i]);
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    using namespace gd::flow;
    options o;
    std::string config, name;
    if (int rc = front(argc, argv, true, o, config, name); rc >= 0) return rc;
    try {
        if (!(o.interval > 0)) throw std::runtime_error("--grid-interval must be positive");
        std::vector<double> axes[3];
        for (int a = 0; a < 3; a++) axes[a] = arange(o.range[a][0], o.range[a][1] + o.interval * 0.1, o.interval);
        std::size_t const nx = axes[0].size(), ny = axes[1].size(), nz = axes[2].size(), G = nx * ny * nz;
        if (G == 0 || G > (1u << 28)) throw std::runtime_error("the grid has " + std::to_string(G) + " points");
        std::vector<double> points(3 * G);
        std::vector<int64_t> indices(3 * G);
        for (std::size_t iy = 0, k = 0; iy < ny; iy++)      // np.meshgrid(x, y, z) ('xy'): y slowest, then x, then z
            for (std::size_t ix = 0; ix < nx; ix++)
                for (std::size_t iz = 0; iz < nz; iz++, k++) {
                    points[3 * k] = axes[0][ix]; points[3 * k + 1] = axes[1][iy]; points[3 * k + 2] = axes[2][iz];
                    indices[3 * k] = (int64_t)ix; indices[3 * k + 1] = (int64_t)iy; indices[3 * k + 2] = (int64_t)iz;
                }
        int64_t const shape[3] = {(int64_t)nx, (int64_t)ny, (int64_t)nz};

        device dev;
        gd::h5::hid file(gd::cli::open_output(o.outfile));
        gd::h5::hid group(gd::cli::require_group(file, "/grid_flow/" + name));
        gd::h5::write_string(group, ".config", config);
        auto samples = gd::h5::read_string_list(group, ".samples");      // incremental analysis: earlier samples stay listed
        gd::cli::put_dataset(group, ".grid/shape", shape, {3}, 8, H5T_NATIVE_INT64, H5T_STD_I64LE, nullptr);
        gd::cli::put_dataset(group, ".grid/points", points.data(), {G, 3}, 8, H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, nullptr);
        gd::cli::put_dataset(group, ".grid/indices", indices.data(), {G, 3}, 8, H5T_NATIVE_INT64, H5T_STD_I64LE, nullptr);
        bool const smooth = o.has_smoothing && o.smoothing > 0;
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            std::string const sample = gd::cli::sample_name(path);
            samples.push_back(sample);
            uint32_t F = 0, N = 0;
            auto const hist = load_history(path, F, N);
            sw.read += sw.lap();
            std::vector<float> flows((std::size_t)F * G * 3);
            std::vector<int32_t> cov((std::size_t)F * G);
            gd::cli::check(gd_flow_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_flow_velocities(dev.h, smooth ? (uint32_t)o.smoothing : 0, (uint32_t)o.delay, nullptr, nullptr));
            gd::cli::check(gd_flow_grid(dev.h, o.radius, points.data(), (uint32_t)G, flows.data(), cov.data()));
            int const factor = scaleoffset_factor(flows);
            sw.compute += sw.lap();
            gd::cli::filters ff;
            ff.scaleoffset_kind = H5Z_SO_FLOAT_DSCALE;
            ff.scaleoffset_factor = factor;
            gd::cli::put_dataset(group, sample + "/flows", flows.data(), {F, G, 3}, 4, H5T_NATIVE_FLOAT, H5T_IEEE_F32LE, &ff);
            gd::cli::filters fc;
            fc.scaleoffset_kind = H5Z_SO_INT;
            fc.scaleoffset_factor = H5Z_SO_INT_MINBITS_DEFAULT;
            gd::cli::put_dataset(group, sample + "/coverages", cov.data(), {F, G}, 4, H5T_NATIVE_INT32, H5T_STD_I32LE, &fc);
            H5Fflush(file, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        gd::h5::write_fixed_string_list(group, ".samples", remove_duplicates(samples));
        sw.write += sw.lap();
        sw.report("gd_grid_flow");
    } catch (std::exception const &e) {
        std::fprintf(stderr, "gd_grid_flow: error: %s\n", e.what());
        return 1;
    }
    return 0;
}
