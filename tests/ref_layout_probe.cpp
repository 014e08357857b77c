// Stand-alone host program of tests/test_walk_tree.py: applies layout.h's reference helpers to every 32-bit reference of the
// file named on the command line and prints "kind record first count" for each, one line per reference.
#include <cstdio>
#include <vector>

#include "../rayrs_amd/csrc/layout.h"

using namespace rayrs;

// the builder's side is the inverse of the walks' side
static_assert(ref_kind(record_ref(0x2abcdefu)) == REF_INTERIOR && ref_record(record_ref(0x2abcdefu)) == 0x2abcdefu, "record_ref");
static_assert(ref_kind(group_ref(0xfffffffu, 4u)) == REF_RANGE && ref_first(group_ref(0xfffffffu, 4u)) == 0xfffffffu &&
                  ref_count(group_ref(0xfffffffu, 4u)) == 4u, "group_ref");
static_assert(ref_kind(group_ref(7u, 1u, REF_SINGLE)) == REF_SINGLE && ref_first(group_ref(7u, 1u, REF_SINGLE)) == 7u &&
                  ref_count(group_ref(7u, 1u, REF_SINGLE)) == 1u, "group_ref of a direct leaf");
static_assert(group_ref(0u, 1u) == REF_LEAF_BASE && record_ref(0x3fffffffu) == REF_LEAF_BASE - 1u, "REF_LEAF_BASE");
static_assert(ref_kind(REF_UNUSED) == REF_NONE && REF_UNUSED >= REF_LEAF_BASE, "REF_UNUSED");

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> refs;
    uint32_t r;
    while (std::fread(&r, sizeof(r), 1, f) == 1) refs.push_back(r);
    std::fclose(f);
    for (uint32_t ref : refs) std::printf("%u %u %u %u\n", ref_kind(ref), ref_record(ref), ref_first(ref), ref_count(ref));
    return 0;
}
