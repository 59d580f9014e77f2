// gd_bins_cli.hpp -- what gd_distance_map, gd_covariance_map and gd_gyration share: the bins of their maps (--rebin-rate K, --by-chain, --chains
// a,b,...), the --frames FIRST:COUNT window, and the runs of consecutive selected bins that one rectangle call each serves.
#pragma once
#include "gd_lag_cli.hpp"

namespace gd {
namespace binscli {

inline std::vector<std::string> split(std::string const &v)
{
    std::vector<std::string> out;
    std::size_t at = 0;
    while (at <= v.size()) {
        auto const comma = std::min(v.find(',', at), v.size());
        out.push_back(v.substr(at, comma - at));
        at = comma + 1;
    }
    return out;
}

// --chains a,b,...: names, none empty, none twice
inline bool parse_chains(std::string const &v, std::vector<std::string> &out)
{
    out = split(v);
    for (auto const &s : out)
        if (s.empty() || std::count(out.begin(), out.end(), s) != 1) return false;
    return true;
}

// --frames FIRST:COUNT, COUNT of at least 1
inline bool parse_frames(std::string const &v, long &first, long &count)
{
    auto const colon = v.find(':');
    return colon != std::string::npos && gd::cli::parse_int(v.substr(0, colon), first) && gd::cli::parse_int(v.substr(colon + 1), count) && first >= 0 &&
           count >= 1 && first <= 0xffffffffl && count <= 0xffffffffl;
}

struct bin_options {      // --rebin-rate, --by-chain, --chains
    long rate = 1;
    bool by_chain = false;
    std::vector<std::string> chains;
};

// "" or why the two bin options exclude each other (argparse's wording)
inline std::string conflict(bin_options const &o) { return o.by_chain && o.rate != 1 ? "argument --by-chain: not allowed with argument --rebin-rate" : ""; }

struct bin_plan {      // the bins of one trajectory file and the ones selected
    std::vector<uint32_t> bins, bin_chain;      // (B, 2), (B)
    std::vector<uint32_t> selected;             // ascending bin indices
};

// `rate` consecutive beads per bin within each chain; the last bin of a chain is shorter (Dmap.bins_from_chains)
inline void bins_from_chains(std::vector<uint32_t> const &chains, uint32_t rate, bin_plan &p)
{
    for (std::size_t c = 0; c < chains.size() / 2; c++)
        for (uint32_t a = chains[2 * c]; a < chains[2 * c + 1]; a += rate) {
            p.bins.push_back(a);
            p.bins.push_back(std::min<uint64_t>((uint64_t)a + rate, chains[2 * c + 1]));
            p.bin_chain.push_back((uint32_t)c);
        }
}

inline void plan_bins(bin_options const &o, gd::lagcli::layout const &l, std::string const &path, bin_plan &p)
{
    if (o.by_chain) {
        for (std::size_t c = 0; c < l.chains.size() / 2; c++)
            if (l.chains[2 * c] < l.chains[2 * c + 1]) {
                p.bins.push_back(l.chains[2 * c]);
                p.bins.push_back(l.chains[2 * c + 1]);
                p.bin_chain.push_back((uint32_t)c);
            }
    } else {
        bins_from_chains(l.chains, (uint32_t)o.rate, p);
    }
    std::vector<char> wanted(l.chain_names.size(), o.chains.empty());
    for (auto const &name : o.chains) {
        auto const it = std::find(l.chain_names.begin(), l.chain_names.end(), name);
        gd::h5::check(it != l.chain_names.end(), path + ": no chain named " + name);
        wanted[it - l.chain_names.begin()] = 1;
    }
    for (uint32_t b = 0; b < p.bin_chain.size(); b++)
        if (wanted[p.bin_chain[b]]) p.selected.push_back(b);
    gd::h5::check(!p.selected.empty(), path + ": no bin selected");
}

// the runs of consecutive bin indices of `selected`: (place in selected, first bin, length)
struct run {
    std::size_t at;
    uint32_t first, n;
};

inline std::vector<run> runs_of(std::vector<uint32_t> const &selected)
{
    std::vector<run> out;
    for (std::size_t k = 0; k < selected.size(); k++) {
        if (!out.empty() && out.back().first + out.back().n == selected[k]) out.back().n++;
        else out.push_back({k, selected[k], 1});
    }
    return out;
}

inline std::string join_names(std::vector<std::string> const &v)
{
    std::string s;
    for (std::size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + v[k];
    return s;
}

// bins, bin_chain and chain_names of the selected bins, as both programs write them
inline void put_selected(hid_t group, bin_plan const &p, std::vector<std::string> const &chain_names, gd::cli::filters const &f)
{
    std::size_t const S = p.selected.size();
    std::vector<uint32_t> bins(2 * S), bin_chain(S);
    for (std::size_t k = 0; k < S; k++) {
        bins[2 * k] = p.bins[2 * (std::size_t)p.selected[k]];
        bins[2 * k + 1] = p.bins[2 * (std::size_t)p.selected[k] + 1];
        bin_chain[k] = p.bin_chain[p.selected[k]];
    }
    hsize_t const s = S;
    gd::cli::put(group, "bins", bins.data(), {s, 2}, &f);
    gd::cli::put(group, "bin_chain", bin_chain.data(), {s}, &f);
    gd::h5::unlink_if_present(group, "chain_names");
    gd::h5::write_fixed_string_list(group, "chain_names", chain_names);
}

}  // namespace binscli
}  // namespace gd
