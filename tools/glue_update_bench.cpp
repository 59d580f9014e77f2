// glue_update_bench -- one glue update of R trajectories at N beads, timed by the host clock around the calls, both ways
// (tools/bench_glue.py builds and runs it):
//   host    what gd_1kb --seeds does per update: gd_get_positions, then per replica gd_search_pairs (count, then fetch),
//           gd::glue_binder::update on the replica's std::mt19937_64 and gd_replica_pairs_set
//   device  gd_glue_update (include/gdyn_glue.h)
// on two handles of the same model and state (the force field of gd_1kb with the configuration of tests/test_1kb_driver.py at the same
// volume fraction: random-walk chains in a periodic box, `relax` steps run first), alternating, `steps` integration steps between
// two updates.  Prints one JSON line.
//   glue_update_bench <beads> <replicas> <updates> <relax> <steps>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "../include/gdyn.h"
#include "../include/gdyn_glue.h"
#include "../include/gdyn_replica.h"
#include "../2022a-genome-dynamics_amd/host/gd_1kb_kinetics.hpp"

static void chk(int rc) { if (rc != GD_OK) throw std::runtime_error(gd_last_error()); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Model { uint32_t n, R; double box, reach = 1.6, on = 400.0, off = 300.0; uint32_t max_glues; };

static gd_system *make(Model const &m, std::vector<double> const &xyz)
{
    gd_desc desc{};
    desc.n_beads = m.n; desc.n_replicas = m.R; desc.box_kind = GD_BOX_PERIODIC; desc.box[0] = desc.box[1] = desc.box[2] = m.box;
    gd_system *sys = nullptr;
    chk(gd_create(&desc, &sys));
    std::vector<double> mobility(m.n, 1.0), bending(m.n, 1.0);
    chk(gd_set_bead_params(sys, nullptr, nullptr, mobility.data(), bending.data()));
    gd_pair_softcore pair{};
    pair.eps_a = 2.0; pair.sigma_a = 1.0; pair.p_a = 2; pair.q_a = 3; pair.eps_b = -0.2; pair.sigma_b = 1.5; pair.p_b = 8; pair.q_b = 3;
    chk(gd_set_pair_softcore(sys, &pair));
    gd_bond_params bond{};
    bond.kind = GD_POT_SPRING; bond.k_a = 100.0; bond.l_a = 1.0;
    chk(gd_add_bond_range(sys, &bond, 0, m.n, 1));
    chk(gd_add_bending_range(sys, 0, m.n, 0.0, 1));
    gd_bond_params glue{};
    glue.kind = GD_POT_SOFTCORE; glue.k_a = -3.0; glue.l_a = m.reach; glue.p = 8; glue.q = 3; glue.minimum_image = 1;
    chk(gd_replica_pairs_define(sys, 1, &glue));
    chk(gd_set_positions(sys, xyz.data()));
    chk(gd_begin_phase(sys, nullptr));
    return sys;
}

static void run(gd_system *sys, long steps, uint64_t seed)
{
    if (steps <= 0) return;
    gd_run_desc d{};
    d.temperature = 1.0; d.timestep = 1e-4; d.seed = seed; d.noise_mode = GD_NOISE_PHILOX; d.steps = steps;
    chk(gd_run(sys, &d));
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv)
{
    try {
        if (argc != 6) { std::fprintf(stderr, "usage: glue_update_bench <beads> <replicas> <updates> <relax> <steps>\n"); return 2; }
        Model m{};
        m.n = (uint32_t)std::atol(argv[1]); m.R = (uint32_t)std::atol(argv[2]);
        long const updates = std::atol(argv[3]), relax = std::atol(argv[4]), steps = std::atol(argv[5]);
        m.box = 9.0 * std::cbrt(double(m.n) / 300.0); m.max_glues = std::max<uint32_t>(m.n / 10, 1);
        std::vector<double> xyz(3 * (size_t)m.n * m.R);
        std::mt19937_64 rng{12345};
        for (uint32_t r = 0; r < m.R; r++) {      // a unit-step random walk from a uniform point (the box wraps it)
            std::uniform_real_distribution<double> coord{0, m.box};
            std::normal_distribution<double> normal;
            double w[3] = {coord(rng), coord(rng), coord(rng)};
            for (uint32_t i = 0; i < m.n; i++) {
                double *x = &xyz[3 * ((size_t)r * m.n + i)];
                for (int k = 0; k < 3; k++) x[k] = w[k];
                double d[3] = {normal(rng), normal(rng), normal(rng)};
                double const inv = 1 / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                for (int k = 0; k < 3; k++) w[k] += d[k] * inv;
            }
        }
        gd_system *host = make(m, xyz), *dev = make(m, xyz);
        gd_glue_params gp{};
        gp.max_glues = m.max_glues; gp.reach = m.reach; gp.binding_rate = m.on; gp.unbinding_rate = m.off;
        chk(gd_glue_define(dev, 1, &gp));
        std::vector<gd::glue_binder> binders;
        std::vector<std::mt19937_64> gens;
        std::vector<uint64_t> seeds;
        for (uint32_t r = 0; r < m.R; r++) { binders.emplace_back(m.max_glues, m.reach, m.on, m.off, m.box); gens.emplace_back(100 + r); seeds.push_back(100 + r); }
        run(host, relax, 7); run(dev, relax, 7);
        double const leap = 1e-4 * double(std::max<long>(steps, 1));
        std::vector<double> t_host, t_dev, t_get, t_search, t_bind;
        double cand = 0, bound_host = 0, bound_dev = 0;
        for (long u = 0; u < updates; u++) {
            for (int side = 0; side < 2; side++) {
                if ((side ^ int(u & 1)) == 0) {
                    double const t0 = now();
                    chk(gd_get_positions(host, xyz.data()));
                    double const t1 = now();
                    double ts = 0, tb = 0;
                    for (uint32_t r = 0; r < m.R; r++) {
                        double const a = now();
                        uint64_t n = 0;
                        chk(gd_search_pairs(host, r, m.reach, nullptr, 0, &n));
                        std::vector<uint32_t> c(2 * n);
                        if (n) chk(gd_search_pairs(host, r, m.reach, c.data(), n, &n));
                        double const b = now();
                        binders[r].update(leap, xyz.data() + 3 * (size_t)m.n * r, c, gens[r]);
                        std::vector<std::pair<uint32_t, uint32_t>> sorted;
                        for (auto const &g : binders[r].pairs()) sorted.push_back({g.i, g.j});
                        std::sort(sorted.begin(), sorted.end());
                        std::vector<uint32_t> pairs;
                        for (auto const &g : sorted) { pairs.push_back(g.first); pairs.push_back(g.second); }
                        chk(gd_replica_pairs_set(host, 1, r, pairs.data(), (uint32_t)(pairs.size() / 2)));
                        ts += b - a; tb += now() - b;
                        cand += double(n); bound_host += double(pairs.size() / 2);
                    }
                    t_host.push_back(now() - t0); t_get.push_back(t1 - t0); t_search.push_back(ts); t_bind.push_back(tb);
                    run(host, steps, 1000 + (uint64_t)u);
                } else {
                    double const t0 = now();
                    chk(gd_glue_update(dev, leap, (uint64_t)u, seeds.data()));
                    t_dev.push_back(now() - t0);
                    std::vector<uint32_t> counts(m.R);
                    chk(gd_glue_counts(dev, counts.data()));
                    for (auto c : counts) bound_dev += double(c);
                    run(dev, steps, 1000 + (uint64_t)u);
                }
            }
        }
        auto mm = [](std::vector<double> const &v) { return std::make_pair(*std::min_element(v.begin(), v.end()), *std::max_element(v.begin(), v.end())); };
        double const per = double(updates) * m.R;
        std::printf("{\"beads\": %u, \"replicas\": %u, \"updates\": %ld, \"relax_steps\": %ld, \"steps_between\": %ld, \"max_glues\": %u, "
                    "\"candidates_per_bead\": %.3f, \"bound_per_replica_host\": %.1f, \"bound_per_replica_device\": %.1f, "
                    "\"host_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f, \"get_positions\": %.3f, \"searches\": %.3f, \"binder_and_set\": %.3f}, "
                    "\"device_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"host_over_device\": %.2f}\n",
                    m.n, m.R, updates, relax, steps, m.max_glues, cand / per / m.n, bound_host / per, bound_dev / per,
                    1e3 * median(t_host), 1e3 * mm(t_host).first, 1e3 * mm(t_host).second, 1e3 * median(t_get), 1e3 * median(t_search), 1e3 * median(t_bind),
                    1e3 * median(t_dev), 1e3 * mm(t_dev).first, 1e3 * mm(t_dev).second, median(t_host) / median(t_dev));
        gd_destroy(host); gd_destroy(dev);
        return 0;
    } catch (std::exception const &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
