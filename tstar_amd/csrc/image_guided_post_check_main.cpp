// Stand-alone checker of the image-guided post-process (image_guided_post_core.h through tstar_image_guided_postprocess_host)
// on the CPU, for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan image_guided_post_host.cpp image_guided_post_check_main.cpp -o image_guided_post_check
//   image_guided_post_check CASE.bin ...
//
// A case file: int32 B, np, has_scale; float32 threshold, nms_threshold; float32 scores [B, np]; boxes [B, np, 4]; with has_scale
// float32 scale [B, 2]; then the expected float32 alphas [B, np], boxes_xyxy [B, np, 4], uint8 keep [B, np], int32 n_kept [B].
// Every buffer is an exact-size heap block.  One line per file: "... differ=N" (words that differ from the expected outputs), or
// "... refused=truncated" for a file shorter than its header says (such a file must be refused, never read past its end).
// Then the tool's own hostile inputs -- NaN, infinite and huge scores and boxes, NaN / infinite / negative thresholds, np at
// both limits, arguments the entry must refuse without writing -- checked for consistency (keep is 0 / 1, n_kept counts it,
// alphas of kept rows in (0, 1]); one line "hostile runs=N bad=M".  Exit status 1 on any difference.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

extern "C" int tstar_image_guided_postprocess_host(const float* scores, const float* boxes_cxcywh, int B, int np, float threshold,
                                                   float nms_threshold, const float* scale_xy, float* alphas, float* boxes_xyxy,
                                                   uint8_t* keep, int32_t* n_kept);

namespace {

struct Reader {
    const std::vector<uint8_t>& d;
    size_t at = 0;
    bool ok = true;
    template <class T>
    std::vector<T> take(size_t n) {
        std::vector<T> v;
        if (!ok || n > (d.size() - at) / sizeof(T)) { ok = false; return v; }
        v.resize(n);
        if (n) memcpy(v.data(), d.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

// one case file -> words that differ, -1 when the file is refused
long run_file(const char* path, int* B_out, int* np_out) {
    std::vector<uint8_t> bytes;
    if (!read_file(path, &bytes)) return -1;
    Reader r{bytes};
    const std::vector<int32_t> head = r.take<int32_t>(3);
    const std::vector<float> par = r.take<float>(2);
    if (!r.ok || head[0] < 1 || head[0] > 65535 || head[1] < 1 || head[1] > 3600) return -1;
    const size_t B = (size_t)head[0], np = (size_t)head[1];
    *B_out = head[0];
    *np_out = head[1];
    const std::vector<float> scores = r.take<float>(B * np), boxes = r.take<float>(B * np * 4);
    const std::vector<float> scale = head[2] ? r.take<float>(B * 2) : std::vector<float>();
    const std::vector<float> want_a = r.take<float>(B * np), want_x = r.take<float>(B * np * 4);
    const std::vector<uint8_t> want_k = r.take<uint8_t>(B * np);
    const std::vector<int32_t> want_n = r.take<int32_t>(B);
    if (!r.ok || r.at != bytes.size()) return -1;
    std::vector<float> a(B * np), x(B * np * 4);
    std::vector<uint8_t> k(B * np);
    std::vector<int32_t> n(B);
    if (tstar_image_guided_postprocess_host(scores.data(), boxes.data(), head[0], head[1], par[0], par[1], head[2] ? scale.data() : nullptr,
                                            a.data(), x.data(), k.data(), n.data()))
        return 1;
    long differ = 0;
    for (size_t i = 0; i < a.size(); ++i) differ += memcmp(&a[i], &want_a[i], 4) != 0;
    for (size_t i = 0; i < x.size(); ++i) differ += memcmp(&x[i], &want_x[i], 4) != 0;
    for (size_t i = 0; i < k.size(); ++i) differ += k[i] != want_k[i];
    for (size_t i = 0; i < n.size(); ++i) differ += n[i] != want_n[i];
    return differ;
}

uint32_t g_rng = 12345;
uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
float unit() { return (float)(rnd() & 0xFFFF) / 65536.0f; }

// one hostile run -> true when the outputs are inconsistent
bool hostile_run(int B, int np, int flavour, float threshold, float nms) {
    const size_t N = (size_t)B * np;
    std::vector<float> scores(N), boxes(N * 4), scale((size_t)B * 2);
    const float odd[8] = {NAN, INFINITY, -INFINITY, 3.4e38f, -3.4e38f, 0.0f, -0.0f, 1e-45f};
    for (size_t i = 0; i < N; ++i) {
        scores[i] = unit();
        for (int c = 0; c < 4; ++c) boxes[i * 4 + c] = unit();
        if (flavour == 1 && rnd() % 3 == 0) scores[i] = odd[rnd() % 8];
        if (flavour == 2 && rnd() % 3 == 0) boxes[i * 4 + rnd() % 4] = odd[rnd() % 8];
        if (flavour == 3) { scores[i] = odd[rnd() % 8]; for (int c = 0; c < 4; ++c) boxes[i * 4 + c] = odd[rnd() % 8]; }
        if (flavour == 4) { scores[i] = 0.5f; boxes[i * 4] = boxes[i * 4 + 1] = 0.5f; boxes[i * 4 + 2] = boxes[i * 4 + 3] = 0.25f; }   // all ties
    }
    for (float& v : scale) v = flavour == 3 ? odd[rnd() % 8] : 1.0f + 1000.0f * unit();
    std::vector<float> a(N), x(N * 4);
    std::vector<uint8_t> k(N);
    std::vector<int32_t> n((size_t)B);
    if (tstar_image_guided_postprocess_host(scores.data(), boxes.data(), B, np, threshold, nms, scale.data(), a.data(), x.data(), k.data(), n.data()))
        return true;
    for (int b = 0; b < B; ++b) {
        int count = 0;
        for (int p = 0; p < np; ++p) {
            const size_t i = (size_t)b * np + p;
            if (k[i] > 1) return true;
            if (k[i] != (a[i] > 0.0f ? 1 : 0)) return true;
            if (k[i] && !(a[i] <= 1.0f)) return true;
            count += k[i];
        }
        if (count != n[(size_t)b]) return true;
    }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    int bad_total = 0;
    for (int i = 1; i < argc; ++i) {
        int B = 0, np = 0;
        const long differ = run_file(argv[i], &B, &np);
        if (differ < 0) {
            printf("%s refused=truncated\n", argv[i]);
        } else {
            printf("%s B=%d np=%d differ=%ld\n", argv[i], B, np, differ);
            bad_total += differ != 0;
        }
    }
    int runs = 0, bad = 0;
    const float thresholds[5] = {0.0f, 0.5f, NAN, INFINITY, -1.0f};
    const float nmss[6] = {0.3f, 0.0f, -1.0f, NAN, 1.0f, INFINITY};
    const int nps[4] = {1, 2, 97, 3600};
    for (int flavour = 0; flavour < 5; ++flavour)
        for (int ni = 0; ni < 4; ++ni)
            for (int t = 0; t < 3; ++t) {
                const int np = nps[ni], B = np == 3600 ? 1 : 3;
                bad += hostile_run(B, np, flavour, thresholds[(flavour + t) % 5], nmss[(flavour + 2 * t + ni) % 6]);
                ++runs;
            }
    // arguments the entry must refuse, without writing
    {
        float s[4] = {0.5f, 0.4f, 0.3f, 0.2f}, b[16] = {0}, a[4] = {-7, -7, -7, -7}, x[16];
        uint8_t k[4] = {9, 9, 9, 9};
        int32_t n[1] = {-5};
        for (int i = 0; i < 16; ++i) x[i] = -7;
        bad += tstar_image_guided_postprocess_host(nullptr, b, 1, 4, 0, 0.3f, nullptr, a, x, k, n) != 1;
        bad += tstar_image_guided_postprocess_host(s, b, 0, 4, 0, 0.3f, nullptr, a, x, k, n) != 1;
        bad += tstar_image_guided_postprocess_host(s, b, 1, 0, 0, 0.3f, nullptr, a, x, k, n) != 1;
        bad += tstar_image_guided_postprocess_host(s, b, 1, 3601, 0, 0.3f, nullptr, a, x, k, n) != 1;
        bad += tstar_image_guided_postprocess_host(s, b, 1, 4, 0, 0.3f, nullptr, a, x, k, nullptr) != 1;
        bad += a[0] != -7 || x[15] != -7 || k[3] != 9 || n[0] != -5;
        runs += 5;
    }
    printf("hostile runs=%d bad=%d\n", runs, bad);
    return bad_total || bad ? 1 : 0;
}
