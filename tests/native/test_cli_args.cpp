// The option scanner of the analysis programs (host/gd_cli_args.hpp) alone, on the CPU: three tables -- long options only, long
// plus short options with attached values, one flag only -- and the tokens at the edge of the option syntax.  Every argv is a
// heap array of exactly argc pointers, so a scanner that reads argv[argc] is caught by AddressSanitizer.
#include "gd_cli_args.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>

using namespace gd::cli;

namespace {

int failures = 0;

struct result {
    std::string err;
    std::vector<std::pair<std::string, std::string>> seen;      // (key, value) in the order handled
    std::vector<std::string> pos;
};

result scan_line(table const &t, shorts s, std::vector<std::string> const &tokens, std::string const &refuse = "")
{
    int const argc = (int)tokens.size() + 1;
    std::vector<std::unique_ptr<char[]>> store;
    std::unique_ptr<char *[]> argv(new char *[argc]);      // no argv[argc]
    for (int k = 0; k < argc; k++) {
        std::string const &tok = k ? tokens[k - 1] : std::string("prog");
        store.emplace_back(new char[tok.size() + 1]);
        std::memcpy(store.back().get(), tok.c_str(), tok.size() + 1);
        argv[k] = store.back().get();
    }
    result r;
    r.err = scan(argc, argv.get(), t, [&](std::string const &key, std::string const &v) {
        r.seen.emplace_back(key, v);
        return key == refuse ? invalid(v, "int") : std::string();
    }, r.pos, s);
    return r;
}

void expect(bool ok, char const *what, int line)
{
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(x) expect((x), #x, __LINE__)

using tokens = std::vector<std::string>;
using pairs = std::vector<std::pair<std::string, std::string>>;

}  // namespace

int main()
{
    table const longs = {{"--dry-run", kind::flag}, {"--lags", kind::value}, {"--log-lags", kind::value}};
    table const mixed = {{"--dry-run", kind::flag}, {"--binsize", kind::value}, {"-b", kind::value}, {"-o", kind::value}};
    table const flag = {{"--dry-run", kind::flag}};

    // ---- long options only
    {
        auto r = scan_line(longs, shorts::exact, {"--lags", "1,2", "--log-lags=7", "out", "--dry-run", "in"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--lags", "1,2"}, {"--log-lags", "7"}, {"--dry-run", ""}}) && r.pos == (tokens{"out", "in"}));
        // the last token wants a value: nothing past argv[argc - 1] is read
        r = scan_line(longs, shorts::exact, {"out", "--lags"});
        EXPECT(r.err == "argument --lags: expected one argument" && r.seen.empty());
        r = scan_line(longs, shorts::exact, {"--log-lags"});
        EXPECT(r.err == "argument --log-lags: expected one argument");
        // a key that is a prefix of another key, or of which another is a prefix, matches nothing
        r = scan_line(longs, shorts::exact, {"--log", "3"});
        EXPECT(r.err == "unrecognized arguments: --log");
        r = scan_line(longs, shorts::exact, {"--lag=3"});
        EXPECT(r.err == "unrecognized arguments: --lag=3");
        r = scan_line(longs, shorts::exact, {"--lagsx", "3"});
        EXPECT(r.err == "unrecognized arguments: --lagsx");
        r = scan_line(longs, shorts::exact, {"--log-lags", "7"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--log-lags", "7"}}));
        // an empty inline value is a value; the handler's refusal is worded after the key
        r = scan_line(longs, shorts::exact, {"--lags=", "x"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--lags", ""}}) && r.pos == (tokens{"x"}));
        r = scan_line(longs, shorts::exact, {"--lags=", "x"}, "--lags");
        EXPECT(r.err == "argument --lags: invalid int value: ''");
        r = scan_line(longs, shorts::exact, {"--lags", "=", "--lags==", "--lags=a=b"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--lags", "="}, {"--lags", "="}, {"--lags", "a=b"}}));
        // a value is the next token whatever it looks like
        r = scan_line(longs, shorts::exact, {"--lags", "--dry-run"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--lags", "--dry-run"}}));
        // a flag takes no inline value
        r = scan_line(longs, shorts::exact, {"--dry-run=1"});
        EXPECT(r.err == "unrecognized arguments: --dry-run=1");
        // the edge tokens: without short options all but "--=" are positionals
        r = scan_line(longs, shorts::exact, {"--", "-", "-5", "-b", "-b7", "-"});
        EXPECT(r.err.empty() && r.seen.empty() && r.pos == (tokens{"--", "-", "-5", "-b", "-b7", "-"}));
        r = scan_line(longs, shorts::exact, {"--="});
        EXPECT(r.err == "unrecognized arguments: --=");
        r = scan_line(longs, shorts::exact, {"--=x", "y"});
        EXPECT(r.err == "unrecognized arguments: --=x");
        r = scan_line(longs, shorts::exact, {});
        EXPECT(r.err.empty() && r.seen.empty() && r.pos.empty());
        r = scan_line(longs, shorts::exact, {""});
        EXPECT(r.err.empty() && r.pos == (tokens{""}));
    }

    // ---- long and short options; exact: "-o v" only, any other token of one dash is a positional
    {
        auto r = scan_line(mixed, shorts::exact, {"-o", "out", "-oout", "-z", "-b", "5", "--binsize=6"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"-o", "out"}, {"-b", "5"}, {"--binsize", "6"}}) && r.pos == (tokens{"-oout", "-z"}));
        r = scan_line(mixed, shorts::exact, {"in", "-o"});
        EXPECT(r.err == "argument -o: expected one argument");
        r = scan_line(mixed, shorts::exact, {"--", "-", "-5"});
        EXPECT(r.err.empty() && r.pos == (tokens{"--", "-", "-5"}));
    }

    // ---- long and short options with attached values: every token of one dash but "-" and "-5" is an option
    {
        auto r = scan_line(mixed, shorts::attached, {"-b", "5", "-b6", "-oout=1", "--binsize", "7", "--binsize=8", "in", "--dry-run"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"-b", "5"}, {"-b", "6"}, {"-o", "out=1"}, {"--binsize", "7"}, {"--binsize", "8"}, {"--dry-run", ""}}) &&
               r.pos == (tokens{"in"}));
        r = scan_line(mixed, shorts::attached, {"in", "-b"});
        EXPECT(r.err == "argument -b: expected one argument" && r.pos == (tokens{"in"}));
        r = scan_line(mixed, shorts::attached, {"-b", "-5"});      // the value is the next token, a negative number too
        EXPECT(r.err.empty() && r.seen == (pairs{{"-b", "-5"}}));
        r = scan_line(mixed, shorts::attached, {"-b=5"}, "-b");
        EXPECT(r.err == "argument -b: invalid int value: '=5'");
        r = scan_line(mixed, shorts::attached, {"-", "-5", "-5x", "-.5"});
        EXPECT(r.err == "unrecognized arguments: -.5" && r.pos == (tokens{"-", "-5", "-5x"}));
        r = scan_line(mixed, shorts::attached, {"--"});
        EXPECT(r.err == "unrecognized arguments: --");
        r = scan_line(mixed, shorts::attached, {"--="});
        EXPECT(r.err == "unrecognized arguments: --=");
        r = scan_line(mixed, shorts::attached, {"-z"});
        EXPECT(r.err == "unrecognized arguments: -z");
        r = scan_line(mixed, shorts::attached, {"-z1", "in"});
        EXPECT(r.err == "unrecognized arguments: -z1");
        r = scan_line(mixed, shorts::attached, {"--binsiz", "5"});
        EXPECT(r.err == "unrecognized arguments: --binsiz");
        r = scan_line(mixed, shorts::attached, {"--b", "5"});      // "-b" is no prefix of a long key
        EXPECT(r.err == "unrecognized arguments: --b");
    }

    // ---- one flag only
    {
        auto r = scan_line(flag, shorts::exact, {"a", "--dry-run", "b", "--dry-run"});
        EXPECT(r.err.empty() && r.seen == (pairs{{"--dry-run", ""}, {"--dry-run", ""}}) && r.pos == (tokens{"a", "b"}));
        r = scan_line(flag, shorts::exact, {"--dry-run"});      // a flag as the last token needs nothing after it
        EXPECT(r.err.empty() && r.seen.size() == 1);
        r = scan_line(flag, shorts::exact, {"--dry", "--dry-run"});
        EXPECT(r.err == "unrecognized arguments: --dry" && r.seen.empty());
        r = scan_line(flag, shorts::exact, {"a", "--dry-run-now"});
        EXPECT(r.err == "unrecognized arguments: --dry-run-now");
        r = scan_line(flag, shorts::attached, {"--dry-run", "-", "-5", "--"});
        EXPECT(r.err == "unrecognized arguments: --" && r.pos == (tokens{"-", "-5"}));
    }

    // ---- a command word selects the table
    {
        std::vector<std::string> pos;
        char a0[] = "prog", a1[] = "--lags", a2[] = "1", a3[] = "word", a4[] = "--lags", a5[] = "2";
        std::unique_ptr<char *[]> argv(new char *[6]{a0, a1, a2, a3, a4, a5});
        auto by_word = [&](std::vector<std::string> const &p) -> table const & { return p.empty() ? flag : longs; };
        std::string err = scan_by(6, argv.get(), shorts::exact, by_word, [](std::string const &, std::string const &) { return std::string(); }, pos);
        EXPECT(err == "unrecognized arguments: --lags" && pos.empty());
        pos.clear();
        std::unique_ptr<char *[]> after(new char *[3]{a0, a3, a4});
        err = scan_by(3, after.get(), shorts::exact, by_word, [](std::string const &, std::string const &) { return std::string(); }, pos);
        EXPECT(err == "argument --lags: expected one argument" && pos == (tokens{"word"}));
    }

    // ---- the converters and their texts
    {
        long i = 0;
        double d = 0;
        EXPECT(to_int("12", i).empty() && i == 12 && to_int("-3", i).empty() && i == -3);
        EXPECT(to_int("", i) == "invalid value: ''" && to_int("1x", i, "int") == "invalid int value: '1x'");
        EXPECT(to_int("99999999999999999999", i) == "invalid value: '99999999999999999999'");
        EXPECT(to_int("0", i, nullptr, 1, 8) == "invalid value: '0'" && to_int("9", i, nullptr, 1, 8) == "invalid value: '9'" && to_int("8", i, nullptr, 1, 8).empty());
        EXPECT(to_float("1.5", d).empty() && d == 1.5 && to_float("1.5x", d, "float") == "invalid float value: '1.5x'" && to_float("", d) == "invalid value: ''");
    }

    if (failures == 0) std::printf("cli args: ok\n");
    return failures ? 1 : 0;
}
