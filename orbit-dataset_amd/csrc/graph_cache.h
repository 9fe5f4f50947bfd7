// HIP-graph cache of a launch sequence (host only): one instantiated graph per distinct key, replayed from the second sight
// of the key on. Shared by the forward and the training entry points of the network runtime (extractor.h).
#pragma once
#include <cstring>
#include <vector>
#include "common.h"

namespace orbit {

// Key: a plain struct of every pointer and scalar that a launch of the sequence bakes in, compared with memcmp: zero it
// (memset) before filling it so that padding never matters. option_epoch() is part of every key (added here): runtime options
// choose kernels, so a graph never replays kernels chosen under other option values.
// Whether to use a graph at all (options graph / train_graph, the bypass while profiling) is the caller's decision.
template <class Key>
class GraphCache {
public:
    explicit GraphCache(size_t capacity) : capacity_(capacity) {}
    ~GraphCache() { clear(); }
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;

    void clear() {
        for (Entry& e : entries_)
            if (e.exec) (void)hipGraphExecDestroy(e.exec);
        entries_.clear();
    }

    // run_fn(stream) enqueues the sequence and returns ORBIT_OK or an error. The first sight of a key runs it on `s` (eager:
    // that run also performs the one-time kernel attribute set-up); the second captures it on *cap_stream (a private
    // non-default stream, created here on first use and owned by the caller: the legacy default stream, torch's default,
    // cannot be captured), instantiates the graph and launches it on `s`; later sights replay. A key whose capture,
    // instantiation or launch failed is marked dead and runs eagerly from then on; an error of run_fn itself is returned.
    // *replayed tells whether a graph launch (true) or an eager run (false) served the call. The least recently used entry is
    // evicted at capacity.
    template <class F>
    int run(const Key& key, hipStream_t s, hipStream_t* cap_stream, F&& run_fn, bool* replayed) {
        *replayed = false;
        const int epoch = option_epoch();
        Entry* hit = nullptr;
        for (Entry& e : entries_)
            if (e.epoch == epoch && memcmp(&e.key, &key, sizeof(Key)) == 0) hit = &e;
        if (hit == nullptr) {
            if (entries_.size() >= capacity_) {
                size_t lru = 0;
                for (size_t i = 1; i < entries_.size(); ++i)
                    if (entries_[i].stamp < entries_[lru].stamp) lru = i;
                if (entries_[lru].exec) (void)hipGraphExecDestroy(entries_[lru].exec);
                entries_.erase(entries_.begin() + lru);
            }
            Entry e;
            e.key = key, e.epoch = epoch, e.stamp = ++clock_;
            entries_.push_back(e);
            return run_fn(s);
        }
        hit->stamp = ++clock_;
        if (!hit->dead && hit->exec == nullptr) {
            if (int rc = capture(hit, *cap_stream, run_fn)) return rc;
        }
        if (!hit->dead && hipGraphLaunch(hit->exec, s) != hipSuccess) {
            (void)hipGetLastError();
            hit->dead = true;
        }
        if (hit->dead) return run_fn(s);
        *replayed = true;
        return ORBIT_OK;
    }

private:
    struct Entry {
        Key key;
        int epoch = 0;                  // option_epoch() at the first sight
        hipGraphExec_t exec = nullptr;  // nullptr: seen once (ran eagerly), captured at the next sight
        bool dead = false;              // capture failed for this key: stay eager
        unsigned long stamp = 0;
    };

    // fills e->exec or marks e dead; returns run_fn's own error, if any
    template <class F>
    int capture(Entry* e, hipStream_t& cap, F&& run_fn) {
        if ((cap == nullptr && hipStreamCreateWithFlags(&cap, hipStreamNonBlocking) != hipSuccess) ||
            hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            e->dead = true;
            return ORBIT_OK;
        }
        const int rc = run_fn(cap);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(cap, &graph);
        hipGraphExec_t exec = nullptr;
        if (rc == ORBIT_OK && ce == hipSuccess && graph != nullptr &&
            hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec != nullptr) {
            e->exec = exec;
        } else {
            (void)hipGetLastError();
            e->dead = true;
        }
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }

    size_t capacity_;
    std::vector<Entry> entries_;
    unsigned long clock_ = 0;
};

}  // namespace orbit
