// gd_gyration -- gyration tensors and compaction profiles of trajectories on the device (include/gdyn_gyr.h): for every trajectory file
// and every selected frame of a phase, the centre and the centred second-moment sums of every segment (a chain, or with --rebin-rate K a
// domain of K beads within a chain), and with --windows the Rg^2 of sliding windows of w beads along the selected chains, summed over
// the frames.  The reference has no such analysis.  Per input sample, under /gyr/<name>/<sample>/ of the output file, with S the selected
// segments, K the selected frames, N the beads and W the window sizes:
//   segments (S, 2) uint32, segment_chain (S) uint32, chain_names (C) fixed-length strings, frames (K) uint32,
//   centre (K, S, 3), moment (K, S, 6: xx yy zz xy xz yz) and rg2 (K, S) float64         rg2 = ((xx + yy) + zz) / n, the tensor = moment / n
//   with --windows:   windows (W) uint32, sum (W, N) and sum_sq (W, N) float64, count (W, N) uint64, by the window's first bead
//   with --kymograph: kymograph/w_<w> (K, N) float64, Rg^2 of the window of w beads at every selected frame
//   gd_gyration [--name PHASE] [--by-chain | --rebin-rate K] [--chains a,b,...] [--frames FIRST:COUNT] [--frame-stride k]
//               [--windows w1,w2,...] [--kymograph w] [--dry-run] outfile trajfiles...
// The segment outputs are always written; --windows and --kymograph add the profile to them, and a run without either removes what an
// earlier run left of it.  Segments are the chains unless --rebin-rate is given (--by-chain says so aloud); --name, --chains and
// --frames are gd_distance_map's (gd_bins_cli.hpp).  The frames are FIRST + j k of the window.  A window lies inside one selected chain.
// Eigenvalues and axes are the caller's (gyr.py: Gyration.descriptors).  --dry-run prints the plan and, for every trajectory file
// given, its shape, segments and frames; no device is used.
#include "../../include/gdyn_gyr.h"
#include "gd_bins_cli.hpp"

using namespace gd::lagcli;
using namespace gd::binscli;

namespace {

struct options : bin_options {
    std::string name = "interphase";
    long stride = 1, kymograph = 0;
    bool has_rate = false, has_frames = false, dry_run = false;
    long first_frame = 0, n_frames = 0;
    std::vector<uint32_t> windows;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

// --windows w1,w2,...: 1 to GD_GYR_MAX_WINDOWS distinct sizes of 2 to GD_GYR_MAX_WINDOW beads
bool parse_windows(std::string const &v, std::vector<uint32_t> &out)
{
    if (!parse_list(v, out) || out.size() > GD_GYR_MAX_WINDOWS) return false;
    for (uint32_t w : out)
        if (w < 2 || w > GD_GYR_MAX_WINDOW) return false;
    return true;
}

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--by-chain", kind::flag}, {"--name", kind::value}, {"--frames", kind::value},
                                           {"--frame-stride", kind::value}, {"--rebin-rate", kind::value}, {"--chains", kind::value},
                                           {"--windows", kind::value}, {"--kymograph", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--by-chain") return o.by_chain = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--frame-stride") return gd::cli::to_int(v, o.stride, nullptr, 1, 0xffffffffl);
        if (key == "--rebin-rate") return o.has_rate = true, gd::cli::to_int(v, o.rate, nullptr, 1, 1l << 28);
        if (key == "--windows") return gd::cli::valid_if(parse_windows(v, o.windows), v);
        if (key == "--kymograph") return gd::cli::to_int(v, o.kymograph, nullptr, 2, GD_GYR_MAX_WINDOW);
        return gd::cli::valid_if(parse_chains(v, o.chains), v);
    }, pos);
    if (!err.empty()) return 2;
    if (o.by_chain && o.has_rate) { err = "argument --by-chain: not allowed with argument --rebin-rate"; return 2; }
    o.by_chain = !o.has_rate;      // the chains are the segments unless a rate is given
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

struct plan : bin_plan {
    uint32_t first_frame = 0, n_selected = 0;
    std::vector<uint32_t> segments, segment_chain, chains;      // the selected segments (S, 2), (S), and the chains that hold them (., 2)
};

plan make_plan(options const &o, layout const &l, std::string const &path, uint32_t F)
{
    plan p;
    plan_bins(o, l, path, p);
    p.first_frame = o.has_frames ? (uint32_t)o.first_frame : 0;
    uint64_t const n_frames = o.has_frames ? (uint64_t)o.n_frames : F;
    gd::h5::check(p.first_frame + n_frames <= F, path + ": --frames " + std::to_string(p.first_frame) + ":" + std::to_string(n_frames) + " of " +
                                                     std::to_string(F) + " frames");
    p.n_selected = (uint32_t)((n_frames - 1) / (uint64_t)o.stride + 1);
    for (uint32_t b : p.selected) {
        p.segments.push_back(p.bins[2 * (std::size_t)b]);
        p.segments.push_back(p.bins[2 * (std::size_t)b + 1]);
        uint32_t const c = p.bin_chain[b];
        if (p.segment_chain.empty() || p.segment_chain.back() != c) {
            p.chains.push_back(l.chains[2 * (std::size_t)c]);
            p.chains.push_back(l.chains[2 * (std::size_t)c + 1]);
        }
        p.segment_chain.push_back(c);
    }
    return p;
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_gyration [--name PHASE] [--by-chain | --rebin-rate K] [--chains a,b,...] [--frames FIRST:COUNT] [--frame-stride k] "
                        "[--windows w1,w2,...] [--kymograph w] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_gyration", "gd_gyration: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        if (o.dry_run) {
            std::string const chains = join_names(o.chains), windows = join(o.windows);
            std::printf("name\t%s\nsegments\t%s\nchains\t%s\nframes\t%s\nframe stride\t%ld\nwindows\t%s\nkymograph\t%s\n", o.name.c_str(),
                        o.has_rate ? ("rate " + std::to_string(o.rate)).c_str() : "by chain", o.chains.empty() ? "all" : chains.c_str(),
                        o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all", o.stride,
                        o.windows.empty() ? "none" : windows.c_str(), o.kymograph ? std::to_string(o.kymograph).c_str() : "none");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, "all", N);
                plan const p = make_plan(o, l, path, F);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tsegments %zu\tselected %zu\tframes selected %u\n", gd::cli::sample_name(path).c_str(),
                            F, N, l.chains.size() / 2, p.bin_chain.size(), p.selected.size(), p.n_selected);
            }
            return 0;
        }
        gd::cli::handle<gd_gyr, gd_gyr_destroy> dev;
        dev.open([](gd_gyr **h) { gd_gyr_desc const d{0, 0, 0}; return gd_gyr_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, "all", N);
            plan const p = make_plan(o, l, path, F);
            sw.read += sw.lap();
            std::size_t const S = p.segment_chain.size(), K = p.n_selected, W = o.windows.size();
            uint32_t const first = p.first_frame, stride = (uint32_t)o.stride, count = p.n_selected;
            gd::cli::check(gd_gyr_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_gyr_set_segments(dev.h, p.segments.data(), (uint32_t)S));
            gd::cli::check(gd_gyr_set_chains(dev.h, p.chains.data(), (uint32_t)(p.chains.size() / 2)));
            std::vector<double> centre(K * S * 3), moment(K * S * 6), rg2(K * S), sum(W * N), sum_sq(W * N), kymograph(o.kymograph ? K * N : 0);
            std::vector<uint64_t> cnt(W * N);
            gd::cli::check(gd_gyr_tensors(dev.h, first, stride, count, nullptr, centre.data(), moment.data()));
            for (std::size_t k = 0; k < K; k++)
                for (std::size_t s = 0; s < S; s++) {
                    double const *m = &moment[(k * S + s) * 6];
                    rg2[k * S + s] = ((m[0] + m[1]) + m[2]) / (double)(p.segments[2 * s + 1] - p.segments[2 * s]);
                }
            if (W) gd::cli::check(gd_gyr_profile(dev.h, o.windows.data(), (uint32_t)W, first, stride, count, sum.data(), sum_sq.data(), cnt.data()));
            if (o.kymograph) gd::cli::check(gd_gyr_profile_frames(dev.h, (uint32_t)o.kymograph, first, stride, count, kymograph.data()));
            sw.compute += sw.lap();
            std::vector<uint32_t> frames(K);
            for (uint32_t k = 0; k < K; k++) frames[k] = first + k * stride;
            gd::h5::hid group(gd::cli::require_group(out, "/gyr/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const s = S, k = K, n = N, w = W;
            gd::cli::put(group, "segments", p.segments.data(), {s, 2}, &f);
            gd::cli::put(group, "segment_chain", p.segment_chain.data(), {s}, &f);
            gd::h5::unlink_if_present(group, "chain_names");
            gd::h5::write_fixed_string_list(group, "chain_names", l.chain_names);
            gd::cli::put(group, "frames", frames.data(), {k}, &f);
            gd::cli::put(group, "centre", centre.data(), {k, s, 3}, &f);
            gd::cli::put(group, "moment", moment.data(), {k, s, 6}, &f);
            gd::cli::put(group, "rg2", rg2.data(), {k, s}, &f);
            for (char const *name : {"windows", "sum", "sum_sq", "count", "kymograph"}) gd::h5::unlink_if_present(group, name);      // of an earlier run
            if (W) {
                gd::cli::put(group, "windows", o.windows.data(), {w}, &f);
                gd::cli::put(group, "sum", sum.data(), {w, n}, &f);
                gd::cli::put(group, "sum_sq", sum_sq.data(), {w, n}, &f);
                gd::cli::put(group, "count", cnt.data(), {w, n}, &f);
            }
            if (o.kymograph) gd::cli::put(group, "kymograph/w_" + std::to_string(o.kymograph), kymograph.data(), {k, n}, &f);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_gyration");
        return 0;
    });
}
