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
#include <json.hpp>   // nlohmann/json single header

#include <map>

#include "../../include/gdyn_msd.h"
#include "gd_flow_cli.hpp"

namespace {

struct lag_option {      // --lags a,b,... or --log-lags K
    std::vector<uint32_t> list;
    long log_count = 16;
    bool explicit_list = false;
};

struct options {
    std::string name = "interphase", groups = "all";
    lag_option lags, seps;
    bool dry_run = false;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

bool parse_list(std::string const &v, std::vector<uint32_t> &out)
{
    out.clear();
    std::size_t at = 0;
    while (at <= v.size()) {
        auto const comma = std::min(v.find(',', at), v.size());
        long x = 0;
        if (!gd::cli::parse_int(v.substr(at, comma - at), x) || x < 1 || x > 0xffffffffl) return false;
        if (std::find(out.begin(), out.end(), (uint32_t)x) != out.end()) return false;
        out.push_back((uint32_t)x);
        at = comma + 1;
    }
    return !out.empty();
}

// --log-lags K over a sequence whose largest lag is `longest`: K values spaced geometrically over [1, longest], each rounded
// half up, duplicates dropped (tests/msd_restatement.py: log_lags)
std::vector<uint32_t> log_lags(long k, uint32_t longest)
{
    std::vector<uint32_t> out;
    if (longest < 1 || k < 1) return out;
    for (long i = 0; i < k; i++) {
        double const v = k == 1 ? 1.0 : std::floor(std::pow((double)longest, (double)i / (double)(k - 1)) + 0.5);
        uint32_t const u = (uint32_t)std::min(std::max(v, 1.0), (double)longest);
        if (out.empty() || u > out.back()) out.push_back(u);
    }
    return out;
}

std::vector<uint32_t> resolve(lag_option const &o, uint32_t longest) { return o.explicit_list ? o.list : log_lags(o.log_count, longest); }

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

struct layout {      // what a trajectory file says about its beads
    std::vector<uint32_t> chains;              // (C, 2)
    std::vector<std::string> chain_names;
    std::vector<int32_t> group;                // empty: one group of all beads
    std::vector<std::string> group_names;
};

void read_chains(hid_t file, std::string const &path, std::string const &phase, uint32_t N, layout &l)
{
    std::string where;
    for (std::string const &g : {"/snapshots/" + phase + "/metadata", std::string("/metadata")})
        if (where.empty() && H5Lexists(file, g.c_str(), H5P_DEFAULT) > 0 && H5Lexists(file, (g + "/chromosome_ranges").c_str(), H5P_DEFAULT) > 0) where = g;
    if (where.empty()) {
        l.chains = {0, N};
        l.chain_names = {"all"};
        return;
    }
    gd::h5::hid meta(H5Gopen2(file, where.c_str(), H5P_DEFAULT));
    std::size_t rows = 0;
    auto const r = gd::h5::read_array<int>(meta, "chromosome_ranges", 2, H5T_NATIVE_INT, &rows);
    l.chain_names.assign(rows, "");
    for (std::size_t c = 0; c < rows; c++) {
        gd::h5::check(r[2 * c] >= 0 && r[2 * c + 1] >= r[2 * c] && (uint32_t)r[2 * c + 1] <= N && (c == 0 || r[2 * c] >= r[2 * c - 1]),
                      path + ": " + where + "/chromosome_ranges is not an ascending list of ranges of the " + std::to_string(N) + " beads");
        l.chains.push_back((uint32_t)r[2 * c]);
        l.chains.push_back((uint32_t)r[2 * c + 1]);
        l.chain_names[c] = "chain" + std::to_string(c);
    }
    gd::h5::hid rds(H5Dopen2(meta, "chromosome_ranges", H5P_DEFAULT));
    if (H5Aexists(rds, "keys") > 0) {
        gd::h5::hid attr(H5Aopen(rds, "keys", H5P_DEFAULT));
        auto const keys = nlohmann::json::parse(gd::h5::read_string_from(attr, true));
        for (auto it = keys.begin(); it != keys.end(); ++it)
            if (it.value().get<std::size_t>() < rows) l.chain_names[it.value().get<std::size_t>()] = it.key();
    }
}

void read_groups(hid_t file, std::string const &path, std::string const &mode, uint32_t N, layout &l)
{
    if (mode == "all") {
        l.group_names = {"all"};
    } else if (mode == "chains") {
        l.group.assign(N, -1);
        for (std::size_t c = 0; c < l.chains.size() / 2; c++)
            for (uint32_t i = l.chains[2 * c]; i < l.chains[2 * c + 1]; i++) l.group[i] = (int32_t)c;
        l.group_names = l.chain_names;
    } else {      // the distinct values of /metadata/particle_types in ascending order, named by the enum where there is one
        gd::h5::hid ds(H5Dopen2(file, "/metadata/particle_types", H5P_DEFAULT));
        gd::h5::check(ds >= 0, path + ": missing dataset /metadata/particle_types");
        gd::h5::hid type(H5Dget_type(ds)), space(H5Dget_space(ds));
        gd::h5::check(H5Sget_simple_extent_npoints(space) == (hssize_t)N, path + ": particle_types does not have one entry per bead");
        std::vector<int8_t> raw(N);
        gd::h5::check(H5Dread(ds, H5T_NATIVE_INT8, H5S_ALL, H5S_ALL, H5P_DEFAULT, raw.data()) >= 0, "cannot read particle_types");
        std::map<int8_t, int32_t> ids;
        for (int8_t v : raw) ids[v] = 0;
        int32_t next = 0;
        for (auto &kv : ids) {
            kv.second = next++;
            char buf[256] = "";
            int8_t value = kv.first;
            if (H5Tget_class(type) == H5T_ENUM && H5Tget_size(type) == 1 && H5Tenum_nameof(type, &value, buf, sizeof buf) >= 0) l.group_names.push_back(buf);
            else l.group_names.push_back(std::to_string((int)kv.first));
        }
        l.group.resize(N);
        for (uint32_t i = 0; i < N; i++) l.group[i] = ids[raw[i]];
    }
}

layout read_layout(std::string const &path, options const &o, uint32_t N)
{
    layout l;
    gd::h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    gd::h5::check(file >= 0, "cannot open " + path);
    read_chains(file, path, o.name, N, l);
    read_groups(file, path, o.groups, N, l);
    return l;
}

uint32_t longest_chain(layout const &l)
{
    uint32_t m = 0;
    for (std::size_t c = 0; c < l.chains.size() / 2; c++) m = std::max(m, l.chains[2 * c + 1] - l.chains[2 * c]);
    return m;
}

std::string join(std::vector<uint32_t> const &v)
{
    std::string s;
    for (std::size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + std::to_string(v[k]);
    return s;
}

std::string describe(lag_option const &l) { return l.explicit_list ? join(l.list) : "log " + std::to_string(l.log_count); }

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
                layout const l = read_layout(path, o, N);
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
            layout const l = read_layout(path, o, N);
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
