// Host build of the piece list of a host-pointer call (mpc_problem.hpp::step_pieces: what step_host of mpc_capi.hip packs with and mpc_create sizes the staging
// blocks with) for tests/test_step_pieces.py: plain g++, no HIP.  Built as a program it walks the same cases itself (for a run under
// -fsanitize=address,undefined: g++ -std=c++17 -fsanitize=address,undefined step_pieces_host.cpp -o step_pieces && ./step_pieces).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../mpc_local_planner_amd/csrc/mpc_problem.hpp"

enum { HAS_U_PREV = 1, HAS_DT_PREV = 2, HAS_INIT = 4, HAS_RADIUS = 8, HAS_VELOCITY = 16, ALL_FLAGS = 31 };

// One call of B instances with the optional arrays of `flags` on a handle created with `c` for max_batch instances: 0, or why its pieces are wrong (in err)
extern "C" int check_call(const mpc_config* c, int64_t max_batch, int64_t B, int flags, char* err, int errlen) {
    typedef mpc::StepPieces SP;
    const SP cap = mpc::step_pieces(*c, (size_t)max_batch, true, true, true, true, true);
    const SP p = mpc::step_pieces(*c, (size_t)B, flags & HAS_U_PREV, flags & HAS_DT_PREV, flags & HAS_INIT, flags & HAS_RADIUS, flags & HAS_VELOCITY);
    auto fail = [&](const char* what, int i, int j) { snprintf(err, (size_t)errlen, "%s (pieces %d, %d)", what, i, j); return 1; };
    if (p.in_bytes > cap.in_bytes || p.out_bytes > cap.out_bytes) return fail("the call packs more than the capacity computed at max_batch", -1, -1);
    const size_t O = c->max_obstacles > 0 ? (size_t)c->max_obstacles : 0;
    // which pieces the call has: the required ones always, the optional ones as asked for, the obstacle arrays with obstacles, velocities with enable_dynamic_obstacles
    const bool want[SP::N_PIECES] = {true, true, (flags & HAS_U_PREV) != 0, (flags & HAS_DT_PREV) != 0, (flags & HAS_INIT) != 0, (flags & HAS_INIT) != 0, (flags & HAS_INIT) != 0,
                                     O > 0, O > 0, O > 0, O > 0 && (flags & HAS_RADIUS), O > 0 && (flags & HAS_VELOCITY) && c->enable_dynamic_obstacles,
                                     true, true, true, true, true, true};
    for (int i = 0; i < SP::N_PIECES; ++i) {
        if ((p.bytes[i] > 0) != want[i]) return fail("a piece is there that the call does not have, or missing", i, i);
        if (!p.bytes[i]) continue;
        const size_t block = i < SP::N_IN ? p.in_bytes : p.out_bytes;
        if (p.off[i] % 256) return fail("a piece does not start on a 256-byte boundary", i, i);
        if (p.off[i] + p.bytes[i] > block) return fail("a piece ends behind what the copy moves", i, i);
        for (int j = 0; j < i; ++j)
            if (p.bytes[j] && (j < SP::N_IN) == (i < SP::N_IN) && p.off[j] < p.off[i] + p.bytes[i] && p.off[i] < p.off[j] + p.bytes[j]) return fail("two pieces overlap", j, i);
    }
    // the sizes are the arrays' (include/mpc_hip.h): spot checks of the ones that depend on n, O and V
    const size_t n = (size_t)c->n, V = c->max_vertices > 0 ? (size_t)c->max_vertices : 1, b = (size_t)B;
    if (p.bytes[SP::X_OUT] != b * n * 24 || p.bytes[SP::U_OUT] != b * n * 16 || (want[SP::X_INIT] && p.bytes[SP::X_INIT] != b * n * 24) ||
        (O && p.bytes[SP::VERTICES] != b * O * V * 16) || (O && p.bytes[SP::N_VERTICES] != b * O * 4))
        return fail("a piece has not the size of its array", -1, -1);
    return 0;
}

int main() {
    int calls = 0, bad = 0;
    const int n_of[2] = {3, 50}, obst[3][2] = {{0, 1}, {1, 1}, {3, 4}};
    const int64_t max_batch = 16384, B_of[2] = {1, max_batch};
    for (int n : n_of)
        for (const int* ov : obst)
            for (int dyn = 0; dyn < 2; ++dyn)
                for (int64_t B : B_of)
                    for (int flags = 0; flags <= ALL_FLAGS; ++flags) {
                        mpc_config c;
                        memset(&c, 0, sizeof(c));
                        c.n = n; c.max_obstacles = ov[0]; c.max_vertices = ov[1]; c.enable_dynamic_obstacles = dyn;
                        char err[256] = "";
                        ++calls;
                        if (check_call(&c, max_batch, B, flags, err, sizeof(err))) { ++bad; printf("n %d O %d V %d dyn %d B %lld flags %d: %s\n", n, ov[0], ov[1], dyn, (long long)B, flags, err); }
                    }
    printf("%d calls, %d with wrong pieces\n", calls, bad);
    return bad ? 1 : 0;
}
