// The table of csrc/ctx_state.hpp as JSON: {product: {"parents": [direct], "falls": [what is invalidated with it]}}
// (tests/test_call_sequences_host.py compiles this with the host compiler and pins the table to the model of call_sequences.py)
#include <cstdio>

#include "ctx_state.hpp"

using namespace ctx_state;

static void names(const char* key, uint32_t mask, const char* end) {
    std::printf("\"%s\": [", key);
    const char* sep = "";
    for (int j = 0; j < N_PRODUCTS; ++j)
        if (mask >> j & 1u) std::printf("%s\"%s\"", sep, TABLE[j].name), sep = ", ";
    std::printf("]%s", end);
}

int main() {
    std::printf("{");
    for (int i = 0; i < N_PRODUCTS; ++i) {
        std::printf("%s\n  \"%s\": {", i ? "," : "", TABLE[i].name);
        names("parents", TABLE[i].parents, ", ");
        names("falls", falls_with(TABLE[i].product) & ~TABLE[i].product, "}");
    }
    std::printf("\n}\n");
    return 0;
}
