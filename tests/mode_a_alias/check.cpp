// Stand-alone check of jac_alias() (calibration_amd/csrc/reproj_math.hpp) and of the Mode A row layout eval_row_slot()
// (calibration_amd/csrc/eval_layout.hpp): compiled and run by tests/test_mode_a_alias.py with the host compiler.
//
// Alias.  For every chain x camera model, in fp64 and fp32, over a few thousand random observations and parameter sets (skew and
// sensor tilts non-zero):
//   * the entry jac_alias() marks is bit-equal (integer view) to the entry it points at in reproj_point()'s output;
//   * no other pair of live entries is marked: exactly JAC_ALIASED_ROWS = 1 entry, v fy -> u skew, both live by jac_const(),
//     and the entry pointed at is not itself sent elsewhere;
//   * the pair is not constant over the samples.
// Layout.  For every chain and width in use (16, 18, 22, 24):
//   * every logical row has a slot in 0 .. jac_stored_rows(PL) - 1;
//   * exactly one pair of rows shares a slot, the pair jac_alias() names;
//   * the slots used cover that range without a hole, and rows that do not share keep their order;
//   * a constant row's slot is shared with no other row;
//   * eval_row_stored() is false exactly for the constants and the aliased entry, eval_tile_width() is slots x 128.
// Mode A's kernel stores the pair once, so a later edit of reproj_core that separates the two entries must fail here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "eval_layout.hpp"

using namespace cba;

template <typename T> struct Bits;
template <> struct Bits<double> { using type = uint64_t; };
template <> struct Bits<float> { using type = uint32_t; };
template <typename T>
static typename Bits<T>::type bits(T x) {
    typename Bits<T>::type b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

static void random_pose(std::mt19937_64& g, double z, double* p) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    double q[4] = {1.0, 0.15 * U(g), 0.15 * U(g), 0.15 * U(g)};
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) p[i] = q[i] / n;
    p[4] = 0.1 * U(g); p[5] = 0.1 * U(g); p[6] = z + 0.2 * U(g);
}

template <int CHAIN, int MODEL, typename T>
static int check_alias(const char* name, int n_samples) {
    constexpr int PI = IntrSize<MODEL>::value, PL = LocalCols<CHAIN, MODEL>::value, OI = intr_col_offset(CHAIN);
    std::mt19937_64 g(4321 + 16 * CHAIN + 4 * MODEL + sizeof(T));
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    int fails = 0, marked = 0;
    for (int row = 0; row < 2; ++row)
        for (int k = 0; k < PL; ++k) {
            const JacEntry a = jac_alias(CHAIN, MODEL, row, k);
            const bool moved = a.row != row || a.k != k;
            if (moved != jac_aliased(CHAIN, MODEL, row, k)) { std::printf("%s: jac_aliased disagrees at (%d, %d)\n", name, row, k); ++fails; }
            if (!moved) continue;
            ++marked;
            if (row != 1 || k != OI + 1 || a.row != 0 || a.k != OI + 4) {
                std::printf("%s: (%d, %d) -> (%d, %d): not v fy -> u skew\n", name, row, k, a.row, a.k);
                ++fails;
            }
            if (a.row < 0 || a.row > 1 || a.k < 0 || a.k >= PL) { std::printf("%s: (%d, %d) points outside the rows\n", name, row, k); ++fails; continue; }
            if (jac_const(CHAIN, MODEL, row, k) != JAC_LIVE || jac_const(CHAIN, MODEL, a.row, a.k) != JAC_LIVE) {
                std::printf("%s: (%d, %d) -> (%d, %d) involves a constant entry\n", name, row, k, a.row, a.k);
                ++fails;
            }
            if (jac_aliased(CHAIN, MODEL, a.row, a.k)) { std::printf("%s: (%d, %d) points at an entry that is itself sent on\n", name, row, k); ++fails; }
        }
    if (marked != JAC_ALIASED_ROWS || marked != 1) { std::printf("%s: %d entries aliased, expected 1\n", name, marked); ++fails; }
    if (jac_stored_rows(PL) != 2 + 2 * PL - 1) { std::printf("%s: jac_stored_rows(%d) = %d\n", name, PL, jac_stored_rows(PL)); ++fails; }

    bool varies = false;
    typename Bits<T>::type first = 0;
    for (int s = 0; s < n_samples; ++s) {
        // every intrinsic non-zero (skew, tangential terms and sensor tilt included), poses that keep the target in front
        double intr[12] = {800 + 100 * U(g), 820 + 100 * U(g), 640 + 30 * U(g), 360 + 30 * U(g), 0.5 + 0.4 * U(g), 0.1 * U(g), 0.05 * U(g),
                           0.01 * U(g), 1e-3 * U(g), 1e-3 * U(g), 0.05 + 0.04 * U(g), -0.04 + 0.03 * U(g)};
        double pA[7], pB[7], q[7], aux[12], bc[BC_SIZE], sd[SD_SIZE];
        for (double& x : sd) x = 0.0;
        if (MODEL == CAM_SCHEIMPFLUG) scheimpflug_consts(intr, sd);
        random_pose(g, CHAIN == CH_BUNDLE ? 2.5 : 2.0, pA);
        random_pose(g, 0.0, pB);
        random_pose(g, 0.5, q);
        quat_to_rotmat(q, aux);
        for (int i = 0; i < 3; ++i) aux[9 + i] = q[4 + i];
        block_consts<CHAIN>(pA, pB, aux, bc);
        T bcT[BC_SIZE], sdT[SD_SIZE], inT[12];
        for (int i = 0; i < BC_SIZE; ++i) bcT[i] = static_cast<T>(bc[i]);
        for (int i = 0; i < SD_SIZE; ++i) sdT[i] = static_cast<T>(sd[i]);
        for (int i = 0; i < PI; ++i) inT[i] = static_cast<T>(intr[i]);
        const T X = static_cast<T>(0.2 * U(g)), Y = static_cast<T>(0.15 * U(g));
        const T uo = static_cast<T>(640 + 300 * U(g)), vo = static_cast<T>(360 + 200 * U(g));
        T r[2], J[2][PL];
        reproj_point<CHAIN, MODEL, T>(bcT, inT, sdT, X, Y, uo, vo, r, J[0], J[1]);
        for (int row = 0; row < 2; ++row)
            for (int k = 0; k < PL; ++k) {
                const JacEntry a = jac_alias(CHAIN, MODEL, row, k);
                if (a.row == row && a.k == k) continue;
                if (bits(J[row][k]) != bits(J[a.row][a.k])) {
                    if (fails < 20) std::printf("%s: sample %d (%d, %d) = %.17g but (%d, %d) = %.17g\n", name, s, row, k,
                                                static_cast<double>(J[row][k]), a.row, a.k, static_cast<double>(J[a.row][a.k]));
                    ++fails;
                }
                if (s == 0) first = bits(J[row][k]);
                else if (bits(J[row][k]) != first) varies = true;
            }
    }
    if (!varies) { std::printf("%s: the aliased entry held the same bits in all %d samples\n", name, n_samples); ++fails; }
    std::printf("%s: alias %s\n", name, fails ? "FAILED" : "ok");
    return fails;
}

static int check_layout(int chain, int model) {
    const int PL = (chain == CH_INTRINSIC ? 6 : 12) + (model == CAM_SCHEIMPFLUG ? 12 : 10);
    const int rows = 2 + 2 * PL, slots = jac_stored_rows(PL);
    int fails = 0;
    auto fail = [&](const char* what, int a, int b) { std::printf("chain %d PL %d: %s (%d, %d)\n", chain, PL, what, a, b); ++fails; };
    std::vector<int> users(static_cast<size_t>(slots), 0);
    for (int row = 0; row < rows; ++row) {
        const int s = eval_row_slot(chain, PL, row);
        if (s < 0 || s >= slots) { fail("slot out of range", row, s); continue; }
        ++users[static_cast<size_t>(s)];
    }
    if (eval_row_slot(chain, PL, 0) != 0 || eval_row_slot(chain, PL, 1) != 1) fail("residual rows moved", 0, 1);
    for (int s = 0; s < slots; ++s)
        if (users[static_cast<size_t>(s)] == 0) fail("hole at slot", s, 0);
    int shared = 0;
    for (int a = 0; a < rows; ++a)
        for (int b = a + 1; b < rows; ++b) {
            const int sa = eval_row_slot(chain, PL, a), sb = eval_row_slot(chain, PL, b);
            const bool moved_a = a >= 2 && jac_aliased(chain, model, (a - 2) / PL, (a - 2) % PL);
            const bool moved_b = b >= 2 && jac_aliased(chain, model, (b - 2) / PL, (b - 2) % PL);
            if (sa != sb) {
                if (!moved_a && !moved_b && sa > sb) fail("rows out of order", a, b);
                continue;
            }
            ++shared;
            // the later row must be the one jac_alias() sends to the earlier
            const JacEntry t = b >= 2 ? jac_alias(chain, model, (b - 2) / PL, (b - 2) % PL) : JacEntry{-1, -1};
            if (a < 2 || !moved_b || 2 + t.row * PL + t.k != a) fail("rows share a slot that jac_alias does not pair", a, b);
            for (int x : {a, b})
                if (x < 2 || jac_const(chain, model, (x - 2) / PL, (x - 2) % PL) != JAC_LIVE) fail("a constant or residual row shares its slot", x, sa);
        }
    if (shared != 1) fail("pairs of rows sharing a slot", shared, 1);
    int skipped = 0;
    for (int row = 0; row < 2; ++row)
        for (int k = 0; k < PL; ++k) {
            const bool st = eval_row_stored(chain, model, row, k);
            if (st != (jac_const(chain, model, row, k) == JAC_LIVE && !jac_aliased(chain, model, row, k))) fail("eval_row_stored", row, k);
            skipped += !st;
        }
    if (skipped != JAC_CONST_ROWS + JAC_ALIASED_ROWS) fail("rows the kernel skips", skipped, JAC_CONST_ROWS + JAC_ALIASED_ROWS);
    if (eval_tile_width(PL) != static_cast<int64_t>(slots) * TILE_A || TILE_A != 128) fail("tile width", static_cast<int>(eval_tile_width(PL)), slots);
    if (eval_alias_row(chain, PL) != 2 + PL + intr_col_offset(chain) + 1) fail("eval_alias_row", eval_alias_row(chain, PL), 0);
    std::printf("chain %d PL %d: layout %s (%d rows in %d slots)\n", chain, PL, fails ? "FAILED" : "ok", rows, slots);
    return fails;
}

// "table": one line "chain model row column to_row to_column" per entry jac_alias() sends elsewhere (the GPU tests read the
// positions from here instead of restating them)
static void print_table() {
    for (int chain = 0; chain < 3; ++chain)
        for (int model = 0; model < 2; ++model) {
            const int PL = (chain == CH_INTRINSIC ? 6 : 12) + (model == CAM_SCHEIMPFLUG ? 12 : 10);
            for (int row = 0; row < 2; ++row)
                for (int k = 0; k < PL; ++k)
                    if (jac_aliased(chain, model, row, k)) {
                        const JacEntry a = jac_alias(chain, model, row, k);
                        std::printf("%d %d %d %d %d %d\n", chain, model, row, k, a.row, a.k);
                    }
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) { print_table(); return 0; }
    const int n = 3000;
    int fails = 0;
#define BOTH(C, M, NAME) fails += check_alias<C, M, double>(NAME " fp64", n); fails += check_alias<C, M, float>(NAME " fp32", n);
    BOTH(CH_INTRINSIC, CAM_PINHOLE_BC, "intrinsic pinhole")
    BOTH(CH_INTRINSIC, CAM_SCHEIMPFLUG, "intrinsic scheimpflug")
    BOTH(CH_EXTRINSIC, CAM_PINHOLE_BC, "extrinsic pinhole")
    BOTH(CH_EXTRINSIC, CAM_SCHEIMPFLUG, "extrinsic scheimpflug")
    BOTH(CH_BUNDLE, CAM_PINHOLE_BC, "bundle pinhole")
    BOTH(CH_BUNDLE, CAM_SCHEIMPFLUG, "bundle scheimpflug")
#undef BOTH
    for (int chain = 0; chain < 3; ++chain)
        for (int model = 0; model < 2; ++model) fails += check_layout(chain, model);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("all ok\n");
    return 0;
}
