// Stand-alone host program (its own main; plain g++, no HIP) for tests/test_root_uniform_host.py: the root system's wave-uniform form
// (mpc_core.hpp::riccati_root_uniform: exchanges as branches around row swaps, flags read once) against riccati_root_shape<true, 7>, the headline shape, BIT FOR BIT in
// the return code, dd and nu -- and one boundary product of the partitioned forward sweep with the factors of every product in both orders (std::fma), which is all
// that differs between the replicated form and the one-component-per-lane form of a lane's chain.
// The program makes its own inputs, prints one line per family ("family cases mismatches codes:<-1>/<0>/<1> ...") and exits with 1 when anything differs.
// A model of the elimination with run-time indices (below) tells which exchanges a system takes and where the pivot compare ties, so that the coverage can be asserted.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../mpc_local_planner_amd/csrc/mpc_core.hpp"

namespace {
using mpc::RicState;

// the 17 words the root system reads: P55, p5, S5[3], W (row-major, symmetric), om[3]
RicState<double> state(const double* in, int neg) {
    RicState<double> V{};
    V.P[5][5] = in[0]; V.p[5] = in[1];
    for (int b = 0; b < 3; ++b) { V.S[5][b] = in[2 + b]; V.om[b] = in[14 + b]; for (int a = 0; a < 3; ++a) V.W[a][b] = in[5 + 3 * a + b]; }
    V.neg = neg;
    return V;
}
uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

// the exchanges of the partial-pivot elimination of the 4 x 5 tableau (unknowns dt, nu_0..2), in the order of the compares: bit k of `taken` = compare k exchanged, bit k
// of `tied` = its two magnitudes were equal (no exchange).  Compares: column 0 rows 1 2 3, column 1 rows 2 3, column 2 row 3.
void exchange_model(const double* in, unsigned& taken, unsigned& tied) {
    double A[4][5];
    const double* W = in + 5;
    A[0][0] = in[0]; A[0][4] = -in[1];
    for (int b = 0; b < 3; ++b) { A[0][1 + b] = in[2 + b]; A[1 + b][0] = in[2 + b]; A[1 + b][4] = -in[14 + b]; for (int a = 0; a < 3; ++a) A[1 + a][1 + b] = W[3 * a + b]; }
    taken = tied = 0;
    int k = 0;
    for (int c = 0; c < 4; ++c) {
        for (int r = c + 1; r < 4; ++r, ++k) {
            const double x = std::fabs(A[r][c]), y = std::fabs(A[c][c]);
            if (x > y) { taken |= 1u << k; for (int b = 0; b < 5; ++b) { const double t = A[c][b]; A[c][b] = A[r][b]; A[r][b] = t; } }
            else if (x == y) tied |= 1u << k;
        }
        const double ip = 1.0 / A[c][c];
        for (int r = c + 1; r < 4; ++r) { const double m = A[r][c] * ip; for (int b = c; b < 5; ++b) A[r][b] -= m * A[c][b]; }
    }
}

struct Tally {
    const char* name;
    long cases = 0, bad = 0, code[3] = {0, 0, 0};
    explicit Tally(const char* n) : name(n) {}
    void line(const char* extra = "") const { std::printf("%s cases=%ld mismatches=%ld codes=%ld/%ld/%ld%s\n", name, cases, bad, code[0], code[1], code[2], extra); }
};

// both forms on one system; the outputs start from a fill, so that what a form does not write is compared too
bool same(const double* in, int neg, Tally& t) {
    const RicState<double> V = state(in, neg);
    double a[4] = {7.0, 7.0, 7.0, 7.0}, b[4] = {7.0, 7.0, 7.0, 7.0};
    const int ra = mpc::riccati_root_shape<true, 7>(V, a[0], a + 1);
    const int rb = mpc::riccati_root_uniform<true, 7>(V, b[0], b + 1);
    bool ok = ra == rb;
    for (int i = 0; i < 4; ++i) ok = ok && bits(a[i]) == bits(b[i]);
    ++t.cases; t.bad += ok ? 0 : 1;
    if (ra >= -1 && ra <= 1) ++t.code[ra + 1];
    if (!ok) std::printf("  MISMATCH in %s: codes %d %d, dd %.17g %.17g\n", t.name, ra, rb, a[0], b[0]);
    return ok;
}

struct Gen {
    std::mt19937_64 rng;
    explicit Gen(uint64_t seed) : rng(seed) {}
    double normal() { return std::normal_distribution<double>(0.0, 1.0)(rng); }
    double uniform(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); }
    int integer(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); }
    // a symmetric system with the inertia the sweep asks for: the nu block negative definite, the dt-dt entry large and positive
    void right_inertia(double* v) {
        double m[3][3];
        for (auto& r : m) for (double& x : r) x = normal();
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { double s = 0; for (int k = 0; k < 3; ++k) s += m[a][k] * m[b][k]; v[5 + 3 * a + b] = -s - (a == b ? 1e-3 : 0.0); }
        v[0] = 5.0 + std::fabs(normal()); v[1] = normal();
        for (int b = 0; b < 3; ++b) { v[2 + b] = normal(); v[14 + b] = normal(); }
    }
    // any symmetric system, every entry scale * a standard normal with a scale of its own choosing
    template <typename Scale> void symmetric(double* v, Scale scale) {
        v[0] = scale() * normal(); v[1] = scale() * normal();
        for (int b = 0; b < 3; ++b) { v[2 + b] = scale() * normal(); v[14 + b] = scale() * normal(); }
        for (int a = 0; a < 3; ++a) for (int b = a; b < 3; ++b) v[5 + 3 * a + b] = v[5 + 3 * b + a] = scale() * normal();
    }
};
}  // namespace

int main() {
    const double special[8] = {0.0, -0.0, 4.9406564584124654e-324, 1e-310, -1e-310, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                               std::numeric_limits<double>::quiet_NaN()};
    bool all = true;
    double v[17];

    {   // every order of exchanges: 2^6 patterns of the six compares, searched for among symmetric systems whose entries spread over four decades
        Tally t("exchange_orders");
        Gen g(20260924);
        bool seen[64] = {};
        int found = 0;
        for (long i = 0; i < 2000000 && found < 64; ++i) {
            g.symmetric(v, [&] { return std::pow(10.0, g.uniform(-2.0, 2.0)); });
            unsigned taken, tied;
            exchange_model(v, taken, tied);
            if (seen[taken]) continue;
            seen[taken] = true; ++found;
            all = same(v, 0, t) && all;
            all = same(v, 1, t) && all;
        }
        char extra[64]; std::snprintf(extra, sizeof extra, " patterns=%d", found);
        t.line(extra);
    }
    {   // exact ties in the pivot compare (no exchange on a tie): small integers, where eliminations stay exact often enough for ties in the later columns too
        Tally t("pivot_ties");
        Gen g(11);
        unsigned tied_at = 0;
        for (int i = 0; i < 20000; ++i) {
            g.symmetric(v, [&] { return 1.0; });
            for (double& x : v) x = (double)(long)std::lround(2.0 * x);
            if (i % 2) { const double s = g.integer(0, 1) ? 1.0 : -1.0; v[2 + g.integer(0, 2)] = s * v[0]; }      // |S5[b]| = |P55|: a tie in column 0
            unsigned taken, tied;
            exchange_model(v, taken, tied);
            if (!tied) continue;
            tied_at |= tied;
            all = same(v, 0, t) && all;
        }
        char extra[64]; std::snprintf(extra, sizeof extra, " tied_compares=0x%x", tied_at);
        t.line(extra);
    }
    {   // a zero, denormal, infinite or NaN pivot at each position: diagonal systems (their pivots ARE the diagonal, in both eliminations) and the same with small couplings
        Tally t("special_pivots");
        Gen g(12);
        for (int pos = 0; pos < 4; ++pos)
            for (double sp : special)
                for (int coupled = 0; coupled < 3; ++coupled) {
                    for (double& x : v) x = 0.0;
                    v[0] = 6.0; v[5] = -1.0; v[9] = -2.0; v[13] = -3.0; v[1] = 0.5;
                    for (int b = 0; b < 3; ++b) v[14 + b] = 0.25 * (b + 1);
                    if (coupled) { for (int b = 0; b < 3; ++b) v[2 + b] = 1e-3 * g.normal(); const double w = 1e-3 * g.normal(); v[6] = v[8] = w; }
                    if (coupled == 2) { const double w = 1e-3 * g.normal(); v[10] = v[12] = w; v[7] = v[11] = -w; }
                    v[pos == 0 ? 0 : 5 + 4 * (pos - 1)] = sp;
                    all = same(v, 0, t) && all;
                }
        // a pivot that the elimination itself makes vanish: W11 - W01^2 / W00 = 0 exactly, and the dt pivot likewise
        for (double& x : v) x = 0.0;
        v[0] = 6.0; v[5] = -1.0; v[6] = v[8] = 1.0; v[9] = -1.0; v[13] = -3.0;
        all = same(v, 0, t) && all;
        for (double& x : v) x = 0.0;
        v[0] = -1.0; v[2] = 1.0; v[5] = -1.0; v[9] = -2.0; v[13] = -3.0;
        all = same(v, 0, t) && all;
        // and a special value in every word of a well-posed system
        for (int w = 0; w < 17; ++w)
            for (double sp : special) { g.right_inertia(v); v[w] = sp; all = same(v, 0, t) && all; }
        t.line();
    }
    {   // inertia one too many and one too few: counted by the sweep (V.neg), and in the system itself
        Tally t("inertia");
        Gen g(13);
        for (int i = 0; i < 2000; ++i) {
            g.right_inertia(v);
            all = same(v, 0, t) && all;
            all = same(v, 1, t) && all;
            all = same(v, -1, t) && all;
            double u[17]; std::memcpy(u, v, sizeof u);
            u[0] = -u[0];                                      // the dt pivot negative: one too many (the coupling too weak to turn it: the nu block's
            for (int b = 0; b < 3; ++b) u[2 + b] *= 1e-3;      //  eigenvalues are below -1e-3, so S' W^-1 S stays below 1e-3 |S|^2 against a dt-dt entry of 5)
            all = same(u, 0, t) && all;
            std::memcpy(u, v, sizeof u);
            const int a = g.integer(0, 2);
            for (int b = 0; b < 3; ++b) if (b != a) u[5 + 3 * a + b] = u[5 + 3 * b + a] = 0.0;
            u[5 + 4 * a] = 1.0 + std::fabs(u[5 + 4 * a]);      // one component's block positive: one too few
            all = same(u, 0, t) && all;
        }
        t.line();
    }
    {
        Tally t("random_well_scaled");
        Gen g(14);
        for (int i = 0; i < 10000; ++i) {
            if (i % 2) g.right_inertia(v); else g.symmetric(v, [] { return 1.0; });
            all = same(v, 0, t) && all;
        }
        t.line();
    }
    {   // entries 1e-12 .. 1e11, each with a magnitude of its own; half of them with the right inertia's signs on the diagonal
        Tally t("random_badly_scaled");
        Gen g(15);
        for (int i = 0; i < 10000; ++i) {
            g.symmetric(v, [&] { return std::pow(10.0, g.uniform(-12.0, 11.0)); });
            if (i % 2) { v[0] = std::fabs(v[0]); for (int a = 0; a < 3; ++a) v[5 + 4 * a] = -std::fabs(v[5 + 4 * a]); }
            all = same(v, 0, t) && all;
        }
        t.line();
    }
    {   // one boundary product: acc = M[6] + sum_j M[j] xi_j + M[5] dd + sum_a M[7 + a] nu_a, every product with its factors in both orders
        Tally t("boundary_product");
        Gen g(16);
        for (int i = 0; i < 10000; ++i) {
            double M[10], x[9];
            for (double& m : M) m = std::pow(10.0, g.uniform(-8.0, 8.0)) * g.normal();
            for (double& e : x) e = std::pow(10.0, g.uniform(-8.0, 8.0)) * g.normal();
            if (i % 100 == 0) M[g.integer(0, 9)] = special[g.integer(0, 7)];
            const int col[9] = {0, 1, 2, 3, 4, 5, 7, 8, 9};
            double a = M[6], b = M[6];
            for (int j = 0; j < 9; ++j) { a = std::fma(M[col[j]], x[j], a); b = std::fma(x[j], M[col[j]], b); }
            ++t.cases; ++t.code[1];
            if (bits(a) != bits(b)) { ++t.bad; all = false; }
        }
        t.line();
    }
    std::printf("%s\n", all ? "ALL EQUAL" : "DIFFERENT");
    return all ? 0 : 1;
}
