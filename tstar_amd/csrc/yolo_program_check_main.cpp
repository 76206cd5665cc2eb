// Stand-alone checker of the YOLO-World program decoder (yolo_program.h), for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan yolo_program_check_main.cpp -o yolo_program_check
//   yolo_program_check PROGRAM_FILE
//
// PROGRAM_FILE (written by tests/test_yolo_program_host.py): nine int32 -- n_blob, n_ops, n_bufs, n_guides, n_levels, input_buf,
// max_batch, the n_anchor and the op count the program must decode to -- then the op, buffer, attention-layer and head-level
// tables (int32) and the blob (float32).  Every table and the blob are held in exact-size heap blocks, so a read one element
// outside is seen by AddressSanitizer.  decode_program is driven over
//   the program as it is: it must decode to the expected n_anchor and op count;
//   one word at a time of every row of every table set to INT_MIN, -1, 0 and INT_MAX, and max_batch and input_buf likewise;
//   the blob cut to every prefix length: a prefix that ends inside a range the program refers to must be refused, a longer one
//   must decode.
// Every call must return a program or a message.  Prints one line; exit status 1 on any difference.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "yolo_program.h"

using namespace tstar;

namespace {

struct Tables {
    std::vector<int32_t> ops, bufs, guides, levels;
    std::vector<float> blob;
    int input_buf = 0, max_batch = 0;
};

// one call on exact-size copies; n_blob floats of the blob
std::string decode(const Tables& t, size_t n_blob, YoloProgram* p) {
    auto exact = [](const auto& v, size_t n) {
        typedef typename std::decay<decltype(v[0])>::type T;
        std::unique_ptr<T[]> b(new T[n ? n : 1]);
        if (n) memcpy(b.get(), v.data(), n * sizeof(T));
        return b;
    };
    const auto ops = exact(t.ops, t.ops.size());
    const auto bufs = exact(t.bufs, t.bufs.size());
    const auto guides = exact(t.guides, t.guides.size());
    const auto levels = exact(t.levels, t.levels.size());
    const auto blob = exact(t.blob, n_blob);
    return decode_program(blob.get(), n_blob, ops.get(), (int)(t.ops.size() / OP_WORDS), OP_WORDS, bufs.get(), (int)(t.bufs.size() / BUF_WORDS),
                          guides.get(), (int)(t.guides.size() / GUIDE_WORDS), levels.get(), (int)(t.levels.size() / LEVEL_WORDS), t.input_buf,
                          t.max_batch, p);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: yolo_program_check PROGRAM_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[9];
    Tables t;
    bool read_ok = fread(hd, sizeof(int32_t), 9, f) == 9 && hd[0] >= 0 && hd[1] >= 0 && hd[2] >= 0 && hd[3] >= 0 && hd[4] >= 0;
    auto rd = [&](auto& v, size_t n) { v.resize(n); read_ok = read_ok && fread(v.data(), sizeof(v[0]), n, f) == n; };
    if (read_ok) {
        rd(t.ops, (size_t)hd[1] * OP_WORDS); rd(t.bufs, (size_t)hd[2] * BUF_WORDS); rd(t.guides, (size_t)hd[3] * GUIDE_WORDS);
        rd(t.levels, (size_t)hd[4] * LEVEL_WORDS); rd(t.blob, (size_t)hd[0]);
    }
    fclose(f);
    if (!read_ok) { fprintf(stderr, "short program file\n"); return 2; }
    t.input_buf = hd[5]; t.max_batch = hd[6];

    int differ = 0, decoded = 0, refused = 0;
    YoloProgram base;
    const std::string e0 = decode(t, t.blob.size(), &base);
    if (!e0.empty() || base.n_anchor != hd[7] || (int)base.ops.size() != hd[8]) {
        fprintf(stderr, "the unmutated program: '%s', n_anchor %d, %zu ops\n", e0.c_str(), base.n_anchor, base.ops.size());
        ++differ;
    }
    auto call = [&](const Tables& m, size_t n_blob) {
        YoloProgram p;
        const std::string e = decode(m, n_blob, &p);
        // a program or a message, never both or neither
        if (e.empty() == p.ops.empty()) { fprintf(stderr, "neither a program nor a message\n"); ++differ; }
        if (e.empty()) ++decoded; else ++refused;
        return e.empty();
    };
    const int32_t extreme[4] = {INT_MIN, -1, 0, INT_MAX};
    std::vector<int32_t> Tables::*const tables[4] = {&Tables::ops, &Tables::bufs, &Tables::guides, &Tables::levels};
    for (auto tab : tables)
        for (size_t i = 0; i < (t.*tab).size(); ++i)
            for (int32_t v : extreme) {
                Tables m = t;
                (m.*tab)[i] = v;
                call(m, m.blob.size());
            }
    for (int32_t v : extreme) {
        Tables m = t;
        m.max_batch = v;
        call(m, m.blob.size());
        m = t;
        m.input_buf = v;
        call(m, m.blob.size());
    }
    // the blob's referenced ranges end at `need`: every shorter prefix cuts one of them
    size_t need = 0;
    auto use = [&](long long off, long long n) { if (off >= 0 && (size_t)(off + n) > need) need = (size_t)(off + n); };
    for (const YoloOp& op : base.ops)
        if (op.kind == OP_CONV) {
            use(op.conv.w_off, (long long)op.conv.cout * op.conv.ks * op.conv.ks * op.conv.cin);
            use(op.conv.b_off, op.conv.cout);
        }
    for (const YoloGuide& g : base.guides) { use(g.w_off, (long long)g.embed * YOLO_TEXT); use(g.b_off, g.embed); use(g.bias_off, g.heads); }
    for (const YoloLevel& l : base.levels) use(l.param_off, 2);
    int cuts = 0;
    for (size_t n = 0; n <= t.blob.size(); ++n, ++cuts)
        if (call(t, n) != (n >= need)) { fprintf(stderr, "blob prefix of %zu floats (the program needs %zu)\n", n, need); ++differ; }
    printf("ops=%zu n_anchor=%d need=%zu cuts=%d decoded=%d refused=%d differ=%d\n", base.ops.size(), base.n_anchor, need, cuts, decoded, refused, differ);
    return differ ? 1 : 0;
}
