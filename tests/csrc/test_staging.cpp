// Host unit test of retinaface_amd/csrc/staging.h: the run rule of the peer / registered uploads and the piece plan of a pipelined
// synchronous upload, on seeded random batches.  Addresses are only compared and offset, never dereferenced.
//   g++ -O1 -std=c++17 -pthread -fsanitize=address,undefined -o test_staging tests/csrc/test_staging.cpp && ./test_staging
#include <cstdio>
#include <random>

#include "../../retinaface_amd/csrc/staging.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct Batch {
    int n = 0;
    std::vector<const uint8_t *> frames;
    std::vector<int> rows, cols, steps, src_dev;
    std::vector<char> empty;
    std::vector<size_t> off_host, off_peer;          // staging offsets as submit() assigns them to host frames / to peer-copied frames
    size_t need_host = 0;
    size_t dense_bytes(int i) const { return (size_t)rows[i] * cols[i] * 3; }
    size_t span(int i) const { return (size_t)(rows[i] - 1) * steps[i] + (size_t)cols[i] * 3; }
    bool dense(int i) const { return steps[i] == cols[i] * 3; }
};

static Batch draw(std::mt19937 &rng) {
    Batch b;
    b.n = 1 + (int)(rng() % 32);
    const bool back_to_back = rng() % 2;             // one buffer, frame after frame (a camera ring, a slice of a batch tensor)
    const bool one_device = rng() % 2;
    static const int aligned[4][2] = {{448, 448}, {896, 1280}, {64, 256}, {1, 256}};      // rows x cols whose dense size is a multiple of 256
    uintptr_t next = 0x100000000ull;
    size_t need_peer = 0;
    for (int i = 0; i < b.n; i++) {
        int rows, cols;
        if (rng() % 3) { const int *a = aligned[rng() % 4]; rows = a[0]; cols = a[1]; }
        else if (rng() % 4 == 0) { rows = 1 + (int)(rng() % 896); cols = 1 + (int)(rng() % 1280); }
        else { rows = 1 + (int)(rng() % 40); cols = 1 + (int)(rng() % 40); }
        const int step = cols * 3 + (rng() % 4 == 0 ? 1 + (int)(rng() % 64) : 0);
        const int kind = (int)(rng() % 12);          // 0: null frame, 1: zero rows, else a frame
        b.rows.push_back(kind == 1 ? 0 : rows); b.cols.push_back(cols); b.steps.push_back(step);
        b.empty.push_back(kind <= 1);
        if (!back_to_back) next += (size_t)(rng() % 3) * 4096 + (rng() % 2) * 17;
        b.frames.push_back(kind == 0 ? nullptr : (const uint8_t *)next);
        b.src_dev.push_back(one_device ? 1 : (int)(rng() % 3) - 1);
        b.off_host.push_back(0); b.off_peer.push_back(0);
        if (kind <= 1) continue;
        next += (size_t)rows * step;
        b.off_host[i] = b.need_host; b.need_host += align256(b.dense_bytes(i));
        if (b.src_dev[i] >= 0) { b.off_peer[i] = need_peer; need_peer += align256(b.span(i)); }
    }
    return b;
}

// walks a chunk the way submit()'s peer branch (peer = true) and upload_registered() do and checks rule (a); returns the frames merged
static int check_runs(const Batch &b, bool peer, bool per_frame) {
    const std::vector<size_t> &off = peer ? b.off_peer : b.off_host;
    auto eligible = [&](int i) { return !b.empty[i] && (peer ? b.src_dev[i] >= 0 : b.dense(i)); };
    auto same = [&](int x, int y) { return !peer || b.src_dev[x] == b.src_dev[y]; };
    std::vector<int> covered, want;
    for (int i = 0; i < b.n; i++) if (eligible(i)) want.push_back(i);
    int merged = 0, prev_start = -1, prev_end = -1;
    size_t prev_bytes = 0;
    for (int i = 0; i < b.n; i++) {
        if (!eligible(i)) continue;
        const rf::FrameRun run = rf::frame_run(b.frames.data(), b.rows.data(), b.cols.data(), b.steps.data(), b.empty.data(), off.data(), i, b.n,
                                               per_frame, same);
        CHECK(run.end > i && run.end <= b.n);
        if (per_frame) CHECK(run.end == i + 1);
        size_t bytes = run.end == i + 1 ? b.span(i) : 0;
        for (int k = i; k < run.end; k++) {
            covered.push_back(k);
            if (run.end == i + 1) break;
            CHECK(eligible(k) && b.dense(k) && same(i, k));
            CHECK(b.frames[k] == b.frames[i] + bytes && off[k] == off[i] + bytes);       // contiguous in the source and in the block
            bytes += b.dense_bytes(k);
        }
        CHECK(run.bytes == bytes);
        // the run before this one ended at i: it stopped for a reason
        if (prev_end == i && !per_frame)
            CHECK(!(b.dense(prev_start) && b.dense(i) && same(prev_start, i) && b.frames[i] == b.frames[prev_start] + prev_bytes &&
                    off[i] == off[prev_start] + prev_bytes));
        merged += run.end - i - 1;
        prev_start = i; prev_end = run.end; prev_bytes = run.bytes;
        i = run.end - 1;
    }
    CHECK(covered == want);
    return merged;
}

// rules (b) and (c) for one piece count; returns the pieces that carry rows
static int check_pieces(const Batch &b, int pieces) {
    uint8_t *const hbase = (uint8_t *)0x7000000000ull;
    const std::vector<rf::StagePiece> plan = rf::stage_piece_plan(b.frames.data(), b.rows.data(), b.cols.data(), b.steps.data(), b.empty.data(),
                                                                  b.off_host.data(), b.n, b.need_host, pieces, hbase);
    CHECK((int)plan.size() == pieces);
    std::vector<std::vector<int>> seen(b.n);
    for (int i = 0; i < b.n; i++) seen[i].assign(b.empty[i] ? 0 : b.rows[i], 0);
    size_t sent = 0, last_dst = 0;
    int nonempty = 0;
    for (const rf::StagePiece &pc : plan) {
        CHECK(pc.sent == sent && pc.end >= pc.sent && pc.end <= b.need_host);             // back to back from 0, never decreasing
        if (pc.jobs.empty()) CHECK(pc.end == pc.sent);
        else nonempty++;
        for (const rf::ParallelCopier::Job &j : pc.jobs) {
            const size_t d = (size_t)(j.dst - hbase);
            int f = -1;
            for (int i = 0; i < b.n; i++) if (!b.empty[i] && d >= b.off_host[i] && d < b.off_host[i] + b.dense_bytes(i)) f = i;
            CHECK(f >= 0);
            if (f < 0) continue;
            const size_t rb = (size_t)b.cols[f] * 3, r = (d - b.off_host[f]) / rb;
            CHECK(d == b.off_host[f] + r * rb && j.row_bytes == rb && j.src_step == (size_t)b.steps[f]);      // dst = off + r * cols * 3
            CHECK(j.src == b.frames[f] + r * b.steps[f]);                                                    // src = frame + r * step
            CHECK(j.rows >= 1 && r + j.rows <= (size_t)b.rows[f]);
            for (size_t k = r; k < r + j.rows && k < seen[f].size(); k++) seen[f][k]++;
            CHECK(d >= last_dst);                                                                            // in order
            last_dst = d + j.rows * rb;
            CHECK(d >= pc.sent && d + j.rows * rb <= pc.end);                                                // inside its piece's range
        }
        sent = pc.end;
    }
    for (int i = 0; i < b.n; i++)
        for (int c : seen[i]) CHECK(c == 1);                                                                 // every row exactly once
    return nonempty;
}

int main() {
    std::mt19937 rng(20);
    int merged = 0, batches = 0, pitched = 0, empties = 0;
    for (int round = 0; round < 300; round++) {
        const Batch b = draw(rng);
        batches++;
        for (int i = 0; i < b.n; i++) { pitched += !b.empty[i] && !b.dense(i); empties += b.empty[i]; }
        merged += check_runs(b, false, false);
        merged += check_runs(b, true, false);
        CHECK(check_runs(b, true, true) == 0);
        for (int pieces : {1, 2, 3, 4, 7, 64}) check_pieces(b, pieces);
    }
    CHECK(batches >= 200 && merged > 100 && pitched > 100 && empties > 100);      // the draw really produces every kind
    {   // ONE large frame is pipelined as well
        Batch b;
        b.n = 1; b.frames = {(const uint8_t *)0x100000000ull}; b.rows = {896}; b.cols = {1280}; b.steps = {1280 * 3}; b.src_dev = {-1};
        b.empty = {0}; b.off_host = {0}; b.off_peer = {0}; b.need_host = align256(b.dense_bytes(0));
        CHECK(check_pieces(b, 4) > 1);
    }
    std::printf(fails ? "FAILED (%d)\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
