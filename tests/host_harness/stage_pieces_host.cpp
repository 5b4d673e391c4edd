// Host build of the layout of a staged host-pointer call (mpc_problem.hpp::stage_layout: what staged_call of mpc_capi.hip places the caller's arrays with in the
// shared staging pair) for tests/test_stage_pieces.py: plain g++, no HIP.  Built as a program it walks piece lists itself (for a run under
// -fsanitize=address,undefined: g++ -std=c++17 -fsanitize=address,undefined stage_pieces_host.cpp -o stage_pieces && ./stage_pieces).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../mpc_local_planner_amd/csrc/mpc_problem.hpp"

static char g_host[1], g_block[1];      // a caller's array and a block's base: addresses only, never read

// One list of `count` pieces: dir[i] a StageDir, bytes[i] its size, given[i] whether the caller passes the array (else NULL).  0, or why the layout is wrong (in err)
extern "C" int check_list(const int* dir, const uint64_t* bytes, const int* given, int count, char* err, int errlen) {
    auto fail = [&](const char* what, int i, int j) { snprintf(err, (size_t)errlen, "%s (pieces %d, %d)", what, i, j); return 1; };
    if (count < 1 || count > mpc::StageLayout::MAX_PIECES) return fail("the list is longer than a layout holds", count, count);
    mpc::StagePiece pc[mpc::StageLayout::MAX_PIECES];
    for (int i = 0; i < count; ++i)
        pc[i] = {given[i] && dir[i] != mpc::STAGE_OUT ? g_host : nullptr, given[i] && dir[i] != mpc::STAGE_IN ? g_host : nullptr, (size_t)bytes[i], dir[i]};
    const mpc::StageLayout L = mpc::stage_layout(pc, count);
    size_t end = 0;
    for (int i = 0; i < count; ++i) {
        const bool want = given[i] && bytes[i] > 0;
        if (L.present[i] != want) return fail("a piece is there that the call does not have, or missing", i, i);
        if (!want) {
            if (L.at(g_block, i) != nullptr) return fail("an absent piece has an address", i, i);
            continue;
        }
        const size_t a = L.off[i], b = a + (size_t)bytes[i];
        if (L.at(g_block, i) != g_block + a) return fail("a piece's address is not the block's plus its offset", i, i);
        if (a % 256) return fail("a piece does not start on a 256-byte boundary", i, i);
        if (b > end) end = b;
        for (int j = 0; j < i; ++j)
            if (L.present[j] && L.off[j] < b && a < L.off[j] + (size_t)bytes[j]) return fail("two pieces overlap", j, i);
        const size_t back_end = L.d2h_begin + L.d2h_bytes;
        if (dir[i] != mpc::STAGE_OUT ? b > L.h2d_bytes : a < L.h2d_bytes) return fail("the copy to the device misses an input or moves an output", i, i);
        if (dir[i] != mpc::STAGE_IN ? (a < L.d2h_begin || b > back_end) : (b > L.d2h_begin && a < back_end)) return fail("the copy back misses an output or moves an input", i, i);
    }
    if (L.bytes != end) return fail("the total is not the end of the last piece", -1, -1);
    if (L.h2d_bytes > L.bytes || L.d2h_begin + L.d2h_bytes > L.bytes) return fail("a copy reaches behind the total", -1, -1);
    return 0;
}

int main() {
    const uint64_t sizes[6] = {0, 1, 255, 256, 257, 16384 * 24};
    int lists = 0, bad = 0;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&rng](unsigned m) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng >> 33) % m; };
    int dir[mpc::StageLayout::MAX_PIECES], given[mpc::StageLayout::MAX_PIECES];
    uint64_t bytes[mpc::StageLayout::MAX_PIECES];
    char err[256] = "";
    auto run = [&](int count) { ++lists; if (check_list(dir, bytes, given, count, err, sizeof(err))) { ++bad; printf("list %d of %d pieces: %s\n", lists, count, err); } };
    for (int a = 0; a < 36; ++a) {      // every single piece, every pair
        dir[0] = a % 3; given[0] = a / 3 % 2; bytes[0] = sizes[a / 6];
        run(1);
        for (int b = 0; b < 36; ++b) { dir[1] = b % 3; given[1] = b / 3 % 2; bytes[1] = sizes[b / 6]; run(2); }
    }
    for (int count = 3; count <= mpc::StageLayout::MAX_PIECES; ++count)
        for (int rep = 0; rep < 400; ++rep) {      // rep < 3: one direction only; then mixed
            for (int i = 0; i < count; ++i) { dir[i] = rep < 3 ? rep : (int)next(3); given[i] = next(4) != 0; bytes[i] = sizes[next(6)]; }
            run(count);
        }
    printf("%d piece lists, %d with a wrong layout\n", lists, bad);
    return bad ? 1 : 0;
}
