// gd_lag_cli.hpp -- what gd_msd, gd_dcorr, gd_distance_map and gd_structure_factor share: the lag lists of their command lines (--lags a,b,... /
// --log-lags K), the periods of --box, and what a trajectory file says about its beads (the chains of chromosome_ranges, the groups
// of particle_types).
#pragma once
#include <json.hpp>   // nlohmann/json single header

#include <map>

#include "gd_flow_cli.hpp"

namespace gd {
namespace lagcli {

struct lag_option {      // --lags a,b,... or --log-lags K
    std::vector<uint32_t> list;
    long log_count = 16;
    bool explicit_list = false;
};

inline bool parse_list(std::string const &v, std::vector<uint32_t> &out)
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

// the handlers of the options the three programs share (gd_cli_args.hpp): "" or why the value will not do
inline std::string lags_or_count(lag_option &l, bool list, std::string const &v)      // --lags a,b,... / --log-lags K, K of 1 to 2^28
{
    l.explicit_list = list && parse_list(v, l.list);
    return list ? gd::cli::valid_if(l.explicit_list, v) : gd::cli::to_int(v, l.log_count, nullptr, 1, 1l << 28);
}

inline std::string phase_name(std::string const &v, std::string &name) { return gd::cli::valid_if(!(name = v).empty() && v.find('/') == std::string::npos, v); }

// --box Lx,Ly,Lz: three positive finite periods
inline bool parse_box(std::string const &v, double box[3])
{
    std::size_t at = 0;
    for (int a = 0; a < 3; a++) {
        auto const comma = a < 2 ? v.find(',', at) : v.size();
        if (comma == std::string::npos || !gd::cli::parse_float(v.substr(at, comma - at), box[a]) || !(box[a] > 0) || !std::isfinite(box[a])) return false;
        at = comma + 1;
    }
    return true;
}

// --log-lags K over a sequence whose largest lag is `longest`: K values spaced geometrically over [1, longest], each rounded
// half up, duplicates dropped (tests/msd_restatement.py: log_lags)
inline std::vector<uint32_t> log_lags(long k, uint32_t longest)
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

inline std::vector<uint32_t> resolve(lag_option const &o, uint32_t longest) { return o.explicit_list ? o.list : log_lags(o.log_count, longest); }

struct layout {      // what a trajectory file says about its beads
    std::vector<uint32_t> chains;              // (C, 2)
    std::vector<std::string> chain_names;
    std::vector<int32_t> group;                // empty: one group of all beads
    std::vector<std::string> group_names;
};

inline void read_chains(hid_t file, std::string const &path, std::string const &phase, uint32_t N, layout &l)
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

inline void read_groups(hid_t file, std::string const &path, std::string const &mode, uint32_t N, layout &l)
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

inline layout read_layout(std::string const &path, std::string const &phase, std::string const &groups, uint32_t N)
{
    layout l;
    gd::h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    gd::h5::check(file >= 0, "cannot open " + path);
    read_chains(file, path, phase, N, l);
    read_groups(file, path, groups, N, l);
    return l;
}

inline uint32_t longest_chain(layout const &l)
{
    uint32_t m = 0;
    for (std::size_t c = 0; c < l.chains.size() / 2; c++) m = std::max(m, l.chains[2 * c + 1] - l.chains[2 * c]);
    return m;
}

inline std::string join(std::vector<uint32_t> const &v)
{
    std::string s;
    for (std::size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + std::to_string(v[k]);
    return s;
}

inline std::string describe(lag_option const &l) { return l.explicit_list ? join(l.list) : "log " + std::to_string(l.log_count); }

}  // namespace lagcli
}  // namespace gd
