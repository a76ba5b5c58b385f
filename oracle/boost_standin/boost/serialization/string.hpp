// Stand-in for the Boost.Serialization header of this name: TEST INFRASTRUCTURE
// ONLY, on the include path of oracle/ref_chain_driver.cpp and ref_asm_driver.cpp only.
// The reference's sam.hpp, cigar.hpp and haplotype.hpp include the Boost header
// but use nothing from it (their serialize() templates are never instantiated);
// what they take from it by accident is a few standard headers, and those are
// all this file holds.
#pragma once
#include <algorithm>
#include <cassert>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include <vector>
