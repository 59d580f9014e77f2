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
    std::vector<std::string> pos;
    for (int k = 1; k < argc; k++) {
        std::string a = argv[k], v;
        if (a.size() > 2 && a.compare(0, 2, "--") == 0) {
            if (a == "--dry-run") { o.dry_run = true; continue; }
            auto eq = a.find('=');
            bool const inline_value = eq != std::string::npos;
            std::string const key = inline_value ? a.substr(0, eq) : a;
            if (key != "--name" && key != "--lags" && key != "--log-lags" && key != "--seps" && key != "--log-seps" && key != "--groups") {
                err = "unrecognized arguments: " + a;
                return 2;
            }
            if (inline_value) v = a.substr(eq + 1);
            else if (k + 1 < argc) v = argv[++k];
            else { err = "argument " + key + ": expected one argument"; return 2; }
            bool ok = true;
            if (key == "--name") ok = !(o.name = v).empty() && v.find('/') == std::string::npos;
            else if (key == "--groups") ok = (o.groups = v) == "all" || v == "types" || v == "chains";
            else {
                lag_option &l = key == "--lags" || key == "--log-lags" ? o.lags : o.seps;
                if (key == "--lags" || key == "--seps") ok = l.explicit_list = parse_list(v, l.list);
                else {
                    ok = gd::cli::parse_int(v, l.log_count) && l.log_count >= 1 && l.log_count <= (1l << 28);
                    l.explicit_list = false;
                }
            }
            if (!ok) { err = "argument " + key + ": invalid value: '" + v + "'"; return 2; }
        } else {
            pos.push_back(a);
        }
    }
    if (o.dry_run && pos.empty()) return 0;
    if (pos.size() < 2) { err = "the following arguments are required: outfile, trajfiles"; return 2; }
    o.outfile = pos[0];
    o.trajfiles.assign(pos.begin() + 1, pos.end());
    return 0;
}

struct device {      // one gd_msd handle; every failure of the library ends the program with its message
    gd_msd *h = nullptr;
    device()
    {
        gd_msd_desc d{0, 0};
        gd::cli::check(gd_msd_create(&d, &h));
    }
    ~device() { gd_msd_destroy(h); }
};

}  // namespace

int main(int argc, char **argv)
{
    options o;
    std::string err;
    if (parse(argc, argv, o, err)) {
        std::fprintf(stderr,
                     "usage: gd_msd [--name PHASE] [--lags a,b,...|--log-lags K] [--seps a,b,...|--log-seps K] [--groups all|types|chains] [--dry-run] "
                     "outfile trajfiles ...\ngd_msd: error: %s\n",
                     err.c_str());
        return 2;
    }
    try {
        H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
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
        device dev;
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
            gd::cli::put_dataset(group, "lags", lags.data(), {L}, 4, H5T_NATIVE_UINT32, H5T_STD_U32LE, nullptr);
            gd::cli::put_dataset(group, "time_sum2", t2.data(), {G, L}, 8, H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, &f);
            gd::cli::put_dataset(group, "time_sum4", t4.data(), {G, L}, 8, H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, &f);
            gd::cli::put_dataset(group, "time_count", tn.data(), {G, L}, 8, H5T_NATIVE_UINT64, H5T_STD_U64LE, &f);
            gd::cli::put_dataset(group, "seps", seps.data(), {S}, 4, H5T_NATIVE_UINT32, H5T_STD_U32LE, nullptr);
            gd::cli::put_dataset(group, "chain_sum2", c2.data(), {C, S}, 8, H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, &f);
            gd::cli::put_dataset(group, "chain_sum4", c4.data(), {C, S}, 8, H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, &f);
            gd::cli::put_dataset(group, "chain_count", cn.data(), {C, S}, 8, H5T_NATIVE_UINT64, H5T_STD_U64LE, &f);
            gd::h5::unlink_if_present(group, "group_names");
            gd::h5::write_fixed_string_list(group, "group_names", l.group_names);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_msd");
    } catch (std::exception const &e) {
        std::fprintf(stderr, "gd_msd: error: %s\n", e.what());
        return 1;
    }
    return 0;
}
