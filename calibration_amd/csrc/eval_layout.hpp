// eval_layout.hpp — where the rows of a Mode A evaluation live in its output buffer.  Plain constexpr functions of the chain and
// the width, free of any device header: engine.hpp includes it, and tests/mode_a_alias/check.cpp compiles it with the host
// compiler alone.
#pragma once
#include <cstdint>

#include "reproj_math.hpp"

namespace cba {

constexpr int TILE_A = 128;  // Mode A: 64 lanes x 2 adjacent observations

// Row slot of the Mode A output: logical row (0, 1 residuals; 2 + k the u Jacobian row of local column k; 2 + PL + k the v row)
// -> which of the jac_stored_rows(PL) = 2 + 2 PL - 1 stored rows holds it.  The kernel, the fill of the constant rows and every
// fetch go through this one function; the layout is private to them.
//   * The v row's fy entry is the u row's skew entry (reproj_math.hpp jac_alias): it resolves to that row's slot, and the rows
//     after it move down by one.  The buffer holds every Jacobian entry of every observation; one slot answers for two rows.
//   * Every other row keeps its place and its order.  The rows k_eval skips (jac_const) stay where they were, as seven gaps of
//     128 in the tile's run.
// Tile-blocked layout out[tile][slot][128]: the slot as it is.  Whole-array columns r[2][ld], J[2 PL - 1][ld]: column slot - 2.
constexpr int eval_alias_row(int chain, int PL) { return 2 + PL + intr_col_offset(chain) + 1; }  // the logical row without a slot of its own
constexpr int eval_row_slot(int chain, int PL, int row) {
    const int gone = eval_alias_row(chain, PL);
    return row == gone ? 2 + intr_col_offset(chain) + 4 : row > gone ? row - 1 : row;
}
// does k_eval store Jacobian entry (row, k) on every pass?  Not a constant (the fill wrote it), not an entry another one holds.
constexpr bool eval_row_stored(int chain, int model, int row, int k) {
    return jac_const(chain, model, row, k) == JAC_LIVE && !jac_aliased(chain, model, row, k);
}
constexpr int64_t eval_tile_width(int PL) { return static_cast<int64_t>(jac_stored_rows(PL)) * TILE_A; }  // elements of one tile's output

}  // namespace cba
