// gd_msd -- the lag statistics of trajectories on the device (include/gdyn_msd.h): for every trajectory file, the sums behind
// MSD(tau) of the beads of each group and behind R2(s) of each chain over all frames of a phase.  The reference has no such
// analysis.  Per input sample, under /msd/<name>/<sample>/ of the output file:
//   lags (L) uint32, time_sum2 / time_sum4 (G, L) float64, time_count (G, L) uint64      MSD = time_sum2 / time_count
//   seps (S) uint32, chain_sum2 / chain_sum4 (C, S) float64, chain_count (C, S) uint64   R2 = chain_sum2 / chain_count
//   group_names (G) fixed-length strings
//   gd_msd [--name PHASE] [--lags a,b,...|--log-lags K] [--seps a,b,...|--log-seps K] [--groups all|types|chains] [--dry-run] outfile trajfiles...
// --name: the phase whose frames are read (/snapshots/PHASE, as load_positions reads them; default interphase) and the name of
// the output group.  Chains: the phase's chromosome_ranges, else the file's, else one chain of all beads.  Groups: all beads
// (default), the values of /metadata/particle_types, or the chains.  Without --lags / --seps: --log-lags 16 / --log-seps 16.
// --dry-run prints the plan and, for every trajectory file given, the lags and separations it resolves to; no device is used.
#include "../../include/gdyn_msd.h"
#include "gd_lag_cli.hpp"

using namespace gd::lagcli;

namespace {

struct options {
    std::string name = "interphase", groups = "all";
    lag_option lags, seps;
    bool dry_run = false;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--name", kind::value}, {"--lags", kind::value}, {"--log-lags", kind::value},
                                           {"--seps", kind::value}, {"--log-seps", kind::value}, {"--groups", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--groups") return gd::cli::valid_if((o.groups = v) == "all" || v == "types" || v == "chains", v);
        return lags_or_count(key == "--lags" || key == "--log-lags" ? o.lags : o.seps, key == "--lags" || key == "--seps", v);
    }, pos);
    if (!err.empty()) return 2;
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_msd [--name PHASE] [--lags a,b,...|--log-lags K] [--seps a,b,...|--log-seps K] [--groups all|types|chains] [--dry-run] "
                        "outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_msd", "gd_msd: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        if (o.dry_run) {
            std::printf("name\t%s\ngroups\t%s\nlags\t%s\nseps\t%s\n", o.name.c_str(), o.groups.c_str(), describe(o.lags).c_str(), describe(o.seps).c_str());
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, o.groups, N);
                std::string const sample = gd::cli::sample_name(path);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tgroups %zu\n", sample.c_str(), F, N, l.chains.size() / 2, l.group_names.size());
                std::printf("lags\t%s\t%s\n", sample.c_str(), join(resolve(o.lags, F - 1)).c_str());
                std::printf("seps\t%s\t%s\n", sample.c_str(), join(resolve(o.seps, std::max(longest_chain(l), 1u) - 1)).c_str());
            }
            return 0;
        }
        gd::cli::handle<gd_msd, gd_msd_destroy> dev;
        dev.open([](gd_msd **h) { gd_msd_desc const d{0, 0}; return gd_msd_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, o.groups, N);
            auto const lags = resolve(o.lags, F - 1), seps = resolve(o.seps, std::max(longest_chain(l), 1u) - 1);
            sw.read += sw.lap();
            uint32_t const G = (uint32_t)l.group_names.size(), C = (uint32_t)(l.chains.size() / 2);
            std::vector<double> t2((std::size_t)G * lags.size()), t4(t2.size()), c2((std::size_t)C * seps.size()), c4(c2.size());
            std::vector<uint64_t> tn(t2.size()), cn(c2.size());
            gd::cli::check(gd_msd_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_msd_set_groups(dev.h, l.group.empty() ? nullptr : l.group.data(), G));
            gd::cli::check(gd_msd_set_chains(dev.h, l.chains.data(), C));
            gd::cli::check(gd_msd_time(dev.h, lags.data(), (uint32_t)lags.size(), t2.data(), t4.data(), tn.data()));
            gd::cli::check(gd_msd_chain(dev.h, seps.data(), (uint32_t)seps.size(), 0, F, c2.data(), c4.data(), cn.data()));
            sw.compute += sw.lap();
            gd::h5::hid group(gd::cli::require_group(out, "/msd/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const L = lags.size(), S = seps.size();
            gd::cli::put(group, "lags", lags.data(), {L}, nullptr);
            gd::cli::put(group, "time_sum2", t2.data(), {G, L}, &f);
            gd::cli::put(group, "time_sum4", t4.data(), {G, L}, &f);
            gd::cli::put(group, "time_count", tn.data(), {G, L}, &f);
            gd::cli::put(group, "seps", seps.data(), {S}, nullptr);
            gd::cli::put(group, "chain_sum2", c2.data(), {C, S}, &f);
            gd::cli::put(group, "chain_sum4", c4.data(), {C, S}, &f);
            gd::cli::put(group, "chain_count", cn.data(), {C, S}, &f);
            gd::h5::unlink_if_present(group, "group_names");
            gd::h5::write_fixed_string_list(group, "group_names", l.group_names);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_msd");
        return 0;
    });
}
