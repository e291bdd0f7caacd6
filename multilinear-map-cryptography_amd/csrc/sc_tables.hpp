// sc_tables.hpp -- what the generic sum-check engine (sumcheck.hip) and the zero-closure fold
// chains (zero_folds.hip) share: the table limit and the kernel argument naming one pass's tables.
#pragma once
#include "bn254.hpp"

namespace tns {

constexpr int MAX_SC_TABLES = 4;

struct ScTables {
  const Fr *in[MAX_SC_TABLES];
  Fr *out[MAX_SC_TABLES];
};

}  // namespace tns
