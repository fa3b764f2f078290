// Tuning and diagnostic switches.
//
// The product library (lib/libsfmx.so) reads no environment variable: there
// SFMX_DIAG_ENV(name) is a null pointer and the variable's name is not even
// compiled in, so a stray variable cannot change what the library computes.
// The diagnostic build (`make diag` -> lib/libsfmx_diag.so, -DSFMX_DIAG) reads
// them: A/B timing of kernel variants, the variant parity tests
// (tests/diag.py loads that library next to the product one), and the
// alternative BA factorization forms.
//
// The matcher's switches (SFMX_SIFT_VARIANT, SFMX_SIFT_P2, SFMX_ORB_VARIANT,
// SFMX_MATCH_BATCHES, SFMX_SCREEN_PERSIST, SFMX_FULL_ROW_GRID) are read in one
// place, resolve_route of matcher.cpp, once per run, into a MatchRoute
// (match_common.hpp) that the run plan keeps and the launchers receive; a
// value it does not list fails the run with SFMX_EINVAL.  The kernels and
// launch sequences only a non-product route reaches are in match_diag.hip,
// which is empty without -DSFMX_DIAG; kernel templates both libraries
// instantiate are in match_device.hpp.
//
// SFMX_BA_POISON=1 (diagnostic build, read with the BA plan's form switches in ba_solver.hip ensure_plan):
// chol_factor fills the LDS buffer of W_k with quiet NaNs before it loads the W_k rows its masks name
// (ba_chol.hpp g_chol_poison), so a product over a row the item never loaded fails every time instead of
// depending on what the previous workgroup left there.
#pragma once

// SFMX_SIFT_VARIANT value (diagnostic build) of the list path with the exact int8 screen and the subset
// pass 2, the product path before the FP6 screen: kept for A/B timing and parity tests.
constexpr int SIFT_VARIANT_INT8_LISTS = 110;
// SFMX_SIFT_VARIANT value (diagnostic build) of the list path with the FP6 screen and the full-row pass 2
// for every forwarded query, the product path before the one-subset certificate: kept for the same uses.
constexpr int SIFT_VARIANT_FP6_FULL = 111;
// SFMX_SIFT_VARIANT value (diagnostic build) of the product path with the FP6 screen in the MFMA shape that
// is not the product's (32 x 32 x 64, sift_screen6w_kernel of match_diag.hip; the product runs 16 x 16 x 128): kept for the same uses.
constexpr int SIFT_VARIANT_FP6_OTHER_SHAPE = 112;
// SFMX_SIFT_VARIANT value (diagnostic build) of the product path with the certified route's pass 2 on
// sift_subset_kernel (one workgroup per pair and subset, rows staged in LDS), the product path before
// sift_rows_kernel: kept for the same uses.
constexpr int SIFT_VARIANT_FP6_SUBSET_WG = 113;

#ifdef SFMX_DIAG
#include <cstdlib>
#define SFMX_DIAG_ENV(name) std::getenv(name)
#else
#define SFMX_DIAG_ENV(name) (static_cast<const char*>(nullptr))
#endif
