// Stand-alone check of jac_const() (calibration_amd/csrc/reproj_math.hpp) against reproj_point(): compiled and run by
// tests/test_mode_a_const_rows.py with the host compiler.  For every chain x camera model, in fp64 and fp32, over a few hundred
// random parameter sets and target points:
//   * every Jacobian entry that jac_const() marks constant is bit-equal to the value Mode A's fill writes (+0.0, not -0.0; 1.0);
//   * no entry it marks live has the same bits in every sample;
//   * exactly JAC_CONST_ROWS = 7 entries are marked, all among the five leading intrinsics columns.
// Run as `check table` it prints the marked positions instead.
// Mode A's kernel does not store the marked rows, so a later edit of reproj_core that makes one of them live must fail here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "reproj_math.hpp"

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
static int check(const char* name, int n_samples) {
    constexpr int PI = IntrSize<MODEL>::value, PL = LocalCols<CHAIN, MODEL>::value, OI = intr_col_offset(CHAIN);
    std::mt19937_64 g(1234 + 16 * CHAIN + 4 * MODEL + sizeof(T));
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    int fails = 0, marked = 0;
    for (int row = 0; row < 2; ++row)
        for (int k = 0; k < PL; ++k) {
            const int c = jac_const(CHAIN, MODEL, row, k);
            if (c == JAC_LIVE) continue;
            ++marked;
            if ((c != JAC_ZERO && c != JAC_ONE) || k < OI || k > OI + 4) {
                std::printf("%s: row %d column %d marked %d outside the leading intrinsics columns\n", name, row, k, c);
                ++fails;
            }
        }
    if (marked != JAC_CONST_ROWS || marked != 7) {
        std::printf("%s: %d entries marked constant, expected 7\n", name, marked);
        ++fails;
    }
    std::vector<typename Bits<T>::type> first(2 * PL);
    std::vector<char> varies(2 * PL, 0);
    for (int s = 0; s < n_samples; ++s) {
        // parameters: every intrinsic non-zero (skew, tangential terms and sensor tilt included), poses that keep the target
        // in front of the camera
        double intr[12] = {800 + 100 * U(g), 820 + 100 * U(g), 640 + 30 * U(g), 360 + 30 * U(g), 0.5 + 0.4 * U(g), 0.1 * U(g), 0.05 * U(g),
                           0.01 * U(g), 1e-3 * U(g), 1e-3 * U(g), 0.05 + 0.04 * U(g), -0.04 + 0.03 * U(g)};
        double pA[7], pB[7], q[7], aux[12], bc[BC_SIZE], sd[SD_SIZE];
        for (double& x : sd) x = 0.0;
        if (MODEL == CAM_SCHEIMPFLUG) scheimpflug_consts(intr, sd);
        random_pose(g, CHAIN == CH_INTRINSIC ? 2.0 : (CHAIN == CH_EXTRINSIC ? 2.0 : 2.5), pA);
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
                const int c = jac_const(CHAIN, MODEL, row, k);
                const auto b = bits(J[row][k]);
                if (c != JAC_LIVE) {
                    const T want = c == JAC_ONE ? T(1) : T(0);
                    if (b != bits(want)) {
                        if (fails < 20) std::printf("%s: sample %d row %d column %d = %.17g, marked constant %d\n", name, s, row, k,
                                                    static_cast<double>(J[row][k]), c);
                        ++fails;
                    }
                } else if (s == 0) {
                    first[row * PL + k] = b;
                } else if (b != first[row * PL + k]) {
                    varies[row * PL + k] = 1;
                }
            }
    }
    for (int row = 0; row < 2; ++row)
        for (int k = 0; k < PL; ++k)
            if (jac_const(CHAIN, MODEL, row, k) == JAC_LIVE && !varies[row * PL + k]) {
                std::printf("%s: row %d column %d is marked live but held the same bits in all %d samples\n", name, row, k, n_samples);
                ++fails;
            }
    std::printf("%s: %s (%d columns, %d marked)\n", name, fails ? "FAILED" : "ok", PL, marked);
    return fails;
}

// "table": one line "chain model row column value" per entry jac_const() marks constant (the GPU tests read the positions from
// here instead of restating them)
static void print_table() {
    for (int chain = 0; chain < 3; ++chain)
        for (int model = 0; model < 2; ++model) {
            const int PL = (chain == CH_INTRINSIC ? 6 : 12) + (model == CAM_SCHEIMPFLUG ? 12 : 10);
            for (int row = 0; row < 2; ++row)
                for (int k = 0; k < PL; ++k)
                    if (jac_const(chain, model, row, k) != JAC_LIVE) std::printf("%d %d %d %d %d\n", chain, model, row, k, jac_const(chain, model, row, k));
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) { print_table(); return 0; }
    const int n = 400;
    int fails = 0;
#define BOTH(C, M, NAME) fails += check<C, M, double>(NAME " fp64", n); fails += check<C, M, float>(NAME " fp32", n);
    BOTH(CH_INTRINSIC, CAM_PINHOLE_BC, "intrinsic pinhole")
    BOTH(CH_INTRINSIC, CAM_SCHEIMPFLUG, "intrinsic scheimpflug")
    BOTH(CH_EXTRINSIC, CAM_PINHOLE_BC, "extrinsic pinhole")
    BOTH(CH_EXTRINSIC, CAM_SCHEIMPFLUG, "extrinsic scheimpflug")
    BOTH(CH_BUNDLE, CAM_PINHOLE_BC, "bundle pinhole")
    BOTH(CH_BUNDLE, CAM_SCHEIMPFLUG, "bundle scheimpflug")
#undef BOTH
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("all ok\n");
    return 0;
}
