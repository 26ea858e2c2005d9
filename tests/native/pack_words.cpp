// The product's canonical view -> packed record conversion (csrc/ge_host.h view_to_words, what ge_batch_write_rooms stores)
// on the host, for tests/test_summary_reference.py to compare with the summary reference's own packer (oracle/summary.py).
//   pack_words <dsl.json> <rounds> <n_players> <views.bin> <words.bin>
// views.bin: ge_room_view[R]; words.bin: R records of words_of(kind) little-endian uint32 each.  Exit 0 = written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../game_engine_amd/csrc/ge_host.h"

using namespace ge;

static bool slurp(const char *path, std::string &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.assign((size_t)len, '\0');
    const bool ok = fread(&out[0], 1, (size_t)len, f) == (size_t)len;
    fclose(f);
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: pack_words <dsl.json> <rounds> <n_players> <views.bin> <words.bin>\n"); return 2; }
    std::string dsl, raw;
    if (!slurp(argv[1], dsl) || !slurp(argv[4], raw)) { fprintf(stderr, "cannot read input\n"); return 1; }
    ge_game_table tb;
    char err[256];
    if (ge_table_compile_json(dsl.data(), dsl.size(), atoi(argv[2]), &tb, err, sizeof err) != GE_OK) { fprintf(stderr, "%s\n", err); return 1; }
    const uint32_t n = (uint32_t)atoi(argv[3]);
    const bool ww = tb.pack == GE_PACK_WEREWOLF;
    const uint32_t kind = ww ? (n <= 8 ? K_WW8 : K_WW12) : (n <= 4 ? K_TT4 : n <= 8 ? K_TT8 : K_TT12);
    const int W = words_of(kind);
    const size_t R = raw.size() / sizeof(ge_room_view);
    if (R * sizeof(ge_room_view) != raw.size()) { fprintf(stderr, "views.bin is not a whole number of views\n"); return 1; }
    std::vector<uint32_t> words(R * (size_t)W);
    for (size_t r = 0; r < R; r++) {
        ge_room_view v;
        memcpy(&v, raw.data() + r * sizeof v, sizeof v);
        view_to_words(kind, v, tb, &words[r * (size_t)W]);
    }
    FILE *f = fopen(argv[5], "wb");
    if (!f || fwrite(words.data(), 4, words.size(), f) != words.size()) { fprintf(stderr, "cannot write output\n"); return 1; }
    fclose(f);
    return 0;
}
