// gd_cli_args.hpp -- the command lines of the analysis programs, by argparse's conventions.  A program lists its options as a
// table of {key, kind}; scan() walks argv once, hands every option to the program's handler as (key, value), collects the
// positionals and words the three messages it owns: unknown option, missing value, bad value.  The handler answers "" or why the
// value will not do, so a range check stands next to the field it fills.  Standard library only.
#pragma once
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <string>
#include <vector>

namespace gd {
namespace cli {

inline bool parse_int(std::string const &s, long &out)
{
    char *end = nullptr;
    errno = 0;
    out = std::strtol(s.c_str(), &end, 10);
    return !s.empty() && errno == 0 && end && *end == '\0';
}

inline bool parse_float(std::string const &s, double &out)
{
    char *end = nullptr;
    out = std::strtod(s.c_str(), &end);
    return !s.empty() && end && *end == '\0';
}

// the bad-value text: "invalid value: 'v'", or with the converter's name "invalid int value: 'v'"
inline std::string invalid(std::string const &v, char const *type = nullptr) { return std::string("invalid ") + (type ? std::string(type) + " " : "") + "value: '" + v + "'"; }
inline std::string valid_if(bool ok, std::string const &v, char const *type = nullptr) { return ok ? std::string() : invalid(v, type); }
inline std::string to_int(std::string const &v, long &out, char const *type = nullptr, long lo = LONG_MIN, long hi = LONG_MAX)
{
    return valid_if(parse_int(v, out) && out >= lo && out <= hi, v, type);
}
inline std::string to_float(std::string const &v, double &out, char const *type = nullptr) { return valid_if(parse_float(v, out), v, type); }

enum class kind { flag, value };
struct option {
    char const *key;      // "--key" or "-k"
    kind k;
};
using table = std::vector<option>;

// how a token of one dash is read.  exact: an option only if it is a key of the table ("-k v"), else a positional.
// attached: every such token is an option, its value may follow at once ("-kv"); "-5" stays a positional
enum class shorts { exact, attached };

inline option const *find(table const &t, std::string const &key)
{
    for (auto const &o : t)
        if (key == o.key) return &o;
    return nullptr;
}

// table_for(positionals so far) is the table in force at a token (a command word may select it); returns "" or the message
template <typename Tables, typename Handler>
std::string scan_by(int argc, char **argv, shorts s, Tables &&table_for, Handler &&on, std::vector<std::string> &positionals)
{
    for (int k = 1; k < argc; k++) {
        std::string const a = argv[k];
        table const &t = table_for(positionals);
        bool const is_long = a.size() > 2 && a.compare(0, 2, "--") == 0;
        bool const is_short = !is_long && a.size() >= 2 && a[0] == '-' && (s == shorts::attached ? !(a[1] >= '0' && a[1] <= '9') : find(t, a) != nullptr);
        if (!is_long && !is_short) {
            positionals.push_back(a);
            continue;
        }
        auto const cut = is_long ? a.find('=') : s == shorts::attached && a.size() > 2 ? (std::size_t)2 : std::string::npos;
        bool const has_value = cut != std::string::npos;
        std::string const key = a.substr(0, cut);
        std::string v = has_value ? a.substr(is_long ? cut + 1 : cut) : std::string();
        option const *o = find(t, key);
        if (!o || (o->k == kind::flag && has_value)) return "unrecognized arguments: " + a;
        if (o->k == kind::value && !has_value) {
            if (k + 1 >= argc) return "argument " + key + ": expected one argument";
            v = argv[++k];
        }
        std::string const why = on(key, v);
        if (!why.empty()) return "argument " + key + ": " + why;
    }
    return std::string();
}

template <typename Handler>
std::string scan(int argc, char **argv, table const &t, Handler &&on, std::vector<std::string> &positionals, shorts s = shorts::exact)
{
    return scan_by(argc, argv, s, [&t](std::vector<std::string> const &) -> table const & { return t; }, on, positionals);
}

}  // namespace cli
}  // namespace gd
