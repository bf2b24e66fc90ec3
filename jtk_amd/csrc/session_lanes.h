// session_lanes.h -- who shares a stream with whom, without HIP: the per-device table of lanes that sessions take their
// streams from, how many lanes a number of hardware queues pays for, and the rule by which the sessions of one lane gather
// their chain kernels into one launch.  Streams that share a hardware queue run in order, so a stream per session buys
// nothing beyond the queues: a slice's 260 ms chain kernel in front of another slice's pair-HMM launches, or six chain
// launches one behind the other where one launch could have carried them all (the chain is latency-bound: a launch lasts as
// long as its slowest chunk, however many chunks it holds).  The streams are whatever the owner keeps per lane (session.hip:
// two hipStream_t and two events; tests/cpp/session_lanes_main.cpp: mock values), made by a callback; the launch is a
// callback too.  No HIP call, no environment, no timer: a plain C++ compiler and a thread sanitizer reach all of it
// (tests/test_session_lanes.py).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <vector>

#define JTK_LANE_MAX_SEGMENTS 8  // sessions in one merged chain launch (the kernels' by-value segment table)
#define JTK_LANE_MAX_LANES 32

// Below 8 queues, which layout?  true: Q / 2 lanes, each with a side stream (the chain's general kernel runs beside its light
// one); false: Q - 1 single-stream lanes (one queue stays with the host's own streams).  Measured on the headline workload at
// Q = 4 (profiles/lanes_timing.txt); the other layout stays reachable through JTK_LC_LANES / JTK_LC_SIDE_STREAM.
#define JTK_LANE_FEW_QUEUES_PAIRED 1

struct LanePlan {
    int max_lanes;  // per device
    bool side;      // a lane's sessions run the general chain kernel on a second stream
};

// `queues`: the hardware queues the process runs on.  From 8 upwards two streams per lane and four queues for the host's own
// streams: with no more sessions than lanes every session has a lane with a side stream to itself, which is what a stream pair
// per session used to be.  forced_lanes (JTK_LC_LANES; 0: not given) and forced_side (JTK_LC_SIDE_STREAM; < 0: not given)
// override either half.
inline LanePlan lane_plan(int queues, int forced_lanes, int forced_side) {
    LanePlan p;
    if (queues >= 8) {
        p.max_lanes = (queues - 4) / 2;
        p.side = true;
    } else if (JTK_LANE_FEW_QUEUES_PAIRED) {
        p.max_lanes = std::max(1, queues / 2);
        p.side = queues >= 2;
    } else {
        p.max_lanes = std::max(1, queues - 1);
        p.side = false;
    }
    if (forced_lanes > 0) p.max_lanes = forced_lanes;
    if (forced_side >= 0) p.side = forced_side != 0;
    p.max_lanes = std::min(p.max_lanes, JTK_LANE_MAX_LANES);
    return p;
}

// The chain launches of one lane.  A session is "in its pass" from enter() to arrive() / withdraw().  arrive() puts the
// session on the pending list; whoever finds nobody in a pass any more launches everything pending, at most
// JTK_LANE_MAX_SEGMENTS members per call of `launch`, and every member returns once its own launch has been made.  The
// launch runs under the lane's mutex: launches of one lane never interleave.  A waiting member waits for lane-mates that are
// in a pass NOW or enter one while it waits; a mate that has arrived cannot enter another pass before its launch, so a member
// waits for at most (members of the lane - 1) passes, and a mate that leaves its pass early (withdraw) is not waited for.
//
// A hold is a plain enter() / withdraw() pair from a caller that is no member (a test, through include/jtk_lc_debug.h): while
// it is held nobody finds the lane empty, so every arriving member pends; on release a waiting member launches everything
// pending in arrival order, at most JTK_LANE_MAX_SEGMENTS per launch.  A member that withdraws under a hold is neither
// launched nor waited for.  in_pass() / pending() / launch_calls() / recent() say what the lane is doing and what it
// launched: the member counts of the last JTK_LANE_LEDGER calls of `launch`, oldest first.
#define JTK_LANE_LEDGER 8
template <class Member>
class LaneGather {
public:
    int in_pass() {
        std::lock_guard<std::mutex> lock(m_);
        return in_pass_;
    }
    int pending() {
        std::lock_guard<std::mutex> lock(m_);
        return (int)pending_.size();
    }
    unsigned long long launch_calls() {
        std::lock_guard<std::mutex> lock(m_);
        return calls_;
    }
    // members[i] of the i-th oldest of the last min(launch_calls(), JTK_LANE_LEDGER) calls; returns their number.  in_pass,
    // pending and calls (any may be null) are read under the same lock.
    int recent(int *members, int *in_pass = nullptr, int *pending = nullptr, unsigned long long *calls = nullptr) {
        std::lock_guard<std::mutex> lock(m_);
        const int have = (int)std::min<unsigned long long>(calls_, JTK_LANE_LEDGER);
        for (int i = 0; i < have; i++) members[i] = ring_[(calls_ - have + i) % JTK_LANE_LEDGER];
        if (in_pass) *in_pass = in_pass_;
        if (pending) *pending = (int)pending_.size();
        if (calls) *calls = calls_;
        return have;
    }
    void enter() {
        std::lock_guard<std::mutex> lock(m_);
        in_pass_++;
    }
    void withdraw() {
        {
            std::lock_guard<std::mutex> lock(m_);
            in_pass_--;
        }
        cv_.notify_all();  // a waiting member may now be the one that launches
    }
    // launch(Member *const *members, int n) -> int; returns what the launch that carried `me` returned
    template <class Launch>
    int arrive(Member *me, Launch &&launch) {
        std::unique_lock<std::mutex> lock(m_);
        in_pass_--;
        Ticket t;
        t.member = me;
        pending_.push_back(&t);
        for (;;) {
            if (t.launched) return t.rc;
            if (in_pass_ == 0) {
                while (!pending_.empty()) {
                    const size_t n = std::min<size_t>(pending_.size(), JTK_LANE_MAX_SEGMENTS);
                    Member *group[JTK_LANE_MAX_SEGMENTS];
                    for (size_t i = 0; i < n; i++) group[i] = pending_[i]->member;
                    ring_[calls_++ % JTK_LANE_LEDGER] = (int)n;
                    const int rc = launch(static_cast<Member *const *>(group), (int)n);
                    for (size_t i = 0; i < n; i++) {
                        pending_[i]->rc = rc;
                        pending_[i]->launched = true;
                    }
                    pending_.erase(pending_.begin(), pending_.begin() + n);
                }
                cv_.notify_all();
                continue;
            }
            cv_.wait(lock);
        }
    }

private:
    struct Ticket {
        Member *member = nullptr;
        bool launched = false;
        int rc = 0;
    };
    std::mutex m_;
    std::condition_variable cv_;
    int in_pass_ = 0;
    std::vector<Ticket *> pending_;  // tickets live on their members' stacks until launched
    unsigned long long calls_ = 0;   // calls of `launch` so far
    int ring_[JTK_LANE_LEDGER] = {}; // their member counts, call c at c % JTK_LANE_LEDGER
};

// a session's pass through its lane's gather: leaves it on every path out of the scope
template <class Member>
struct LanePass {
    LaneGather<Member> *g;
    bool arrived = false;
    explicit LanePass(LaneGather<Member> *gather) : g(gather) {
        if (g) g->enter();
    }
    ~LanePass() {
        if (g && !arrived) g->withdraw();
    }
    LanePass(const LanePass &) = delete;
    LanePass &operator=(const LanePass &) = delete;
    template <class Launch>
    int arrive(Member *me, Launch &&launch) {
        arrived = true;
        return g->arrive(me, launch);
    }
};

// The polish rounds of one lane.  The sessions of a lane queue their rounds on one stream, where they run one behind the
// other although they are independent; a round's kernels are latency-bound once few chunks are still active.  So lane-mates
// that are in their polish phase at the same time put their rounds into ONE launch sequence (the segment-table kernels).
//
// A member is "in its rounds" from enter() to leave() -- the polish phase of a pass, which ends BEFORE the chain point.  At
// every point where it would queue a round (the pass's opening, then each round) it calls arrive() and is parked.  The launch
// is made as soon as every member that is in its rounds is parked and nobody holds the gather: whoever completes that
// condition (the last to arrive, or a parked member woken by a mate that left) calls `launch` for all parked members in
// arrival order, at most JTK_LANE_MAX_SEGMENTS per call and the rest in the next call; a call of one is a table of one
// segment.  Every member returns once its own launch has been made, and goes back to its own
// bookkeeping (it stays exactly one round queued ahead, as without the gather).
//
// Invariants.  No timers: the only waits are on the condition variable.  A member leaves on every path out of its scope
// (RoundPass).  A parked member waits only for members that are in their rounds and NOT parked, i.e. whose host threads are
// running towards arrive() or leave(); such a thread waits for nothing but events of work already queued.  A member at its
// chain point (LaneGather::arrive) has left its rounds before, so the round gather never waits for it, and the chain gather
// waits only for members that this gather lets run: there is no wait cycle.  A hold of the chain gather therefore does not
// stall rounds either.
//
// hold() / release() are an outsider's (a test's, include/jtk_lc_debug.h): while held nothing launches and arriving members
// pend; the release launches once the condition above holds.  step() lets the members parked at that moment launch once,
// whoever else is in its rounds, and leaves the hold in place: that is how a test puts members of different rounds into one
// launch.  launch_calls() / recent() as LaneGather's.
template <class Member>
class RoundGather {
public:
    void enter() {
        std::lock_guard<std::mutex> lock(m_);
        in_rounds_++;
    }
    void leave() {
        {
            std::lock_guard<std::mutex> lock(m_);
            in_rounds_--;
        }
        cv_.notify_all();  // a parked member may now be the one that launches
    }
    void hold() {
        std::lock_guard<std::mutex> lock(m_);
        holds_++;
    }
    bool release() {  // false: not held
        {
            std::lock_guard<std::mutex> lock(m_);
            if (holds_ == 0) return false;
            holds_--;
        }
        cv_.notify_all();
        return true;
    }
    void step() {
        {
            std::lock_guard<std::mutex> lock(m_);
            if (parked_.empty()) return;
            step_ = true;
        }
        cv_.notify_all();
    }
    int in_rounds() {
        std::lock_guard<std::mutex> lock(m_);
        return in_rounds_;
    }
    int parked() {
        std::lock_guard<std::mutex> lock(m_);
        return (int)parked_.size();
    }
    int holds() {
        std::lock_guard<std::mutex> lock(m_);
        return holds_;
    }
    unsigned long long launch_calls() {
        std::lock_guard<std::mutex> lock(m_);
        return calls_;
    }
    int recent(int *members, int *in_rounds = nullptr, int *parked = nullptr, unsigned long long *calls = nullptr, int *holds = nullptr) {
        std::lock_guard<std::mutex> lock(m_);
        const int have = (int)std::min<unsigned long long>(calls_, JTK_LANE_LEDGER);
        for (int i = 0; i < have; i++) members[i] = ring_[(calls_ - have + i) % JTK_LANE_LEDGER];
        if (in_rounds) *in_rounds = in_rounds_;
        if (parked) *parked = (int)parked_.size();
        if (calls) *calls = calls_;
        if (holds) *holds = holds_;
        return have;
    }
    // launch(Member *const *members, int n) -> int, called under the gather's mutex (a lane's round launches never interleave);
    // returns what the launch that carried `me` returned
    template <class Launch>
    int arrive(Member *me, Launch &&launch) {
        std::unique_lock<std::mutex> lock(m_);
        Ticket t;
        t.member = me;
        parked_.push_back(&t);
        for (;;) {
            if (t.launched) return t.rc;
            if (step_ || (holds_ == 0 && (int)parked_.size() == in_rounds_)) {
                step_ = false;
                while (!parked_.empty()) {
                    const size_t n = std::min<size_t>(parked_.size(), JTK_LANE_MAX_SEGMENTS);
                    Member *group[JTK_LANE_MAX_SEGMENTS];
                    for (size_t i = 0; i < n; i++) group[i] = parked_[i]->member;
                    ring_[calls_++ % JTK_LANE_LEDGER] = (int)n;
                    const int rc = launch(static_cast<Member *const *>(group), (int)n);
                    for (size_t i = 0; i < n; i++) {
                        parked_[i]->rc = rc;
                        parked_[i]->launched = true;
                    }
                    parked_.erase(parked_.begin(), parked_.begin() + n);
                }
                cv_.notify_all();
                continue;
            }
            cv_.wait(lock);
        }
    }

private:
    struct Ticket {
        Member *member = nullptr;
        bool launched = false;
        int rc = 0;
    };
    std::mutex m_;
    std::condition_variable cv_;
    int in_rounds_ = 0, holds_ = 0;
    bool step_ = false;
    std::vector<Ticket *> parked_;   // tickets live on their members' stacks until launched
    unsigned long long calls_ = 0;
    int ring_[JTK_LANE_LEDGER] = {};
};

// a session's polish phase in its lane's round gather: leaves it on every path out of the scope
template <class Member>
struct RoundPass {
    RoundGather<Member> *g;
    explicit RoundPass(RoundGather<Member> *gather) : g(gather) {
        if (g) g->enter();
    }
    ~RoundPass() { leave(); }
    RoundPass(const RoundPass &) = delete;
    RoundPass &operator=(const RoundPass &) = delete;
    void leave() {
        if (g) g->leave();
        g = nullptr;
    }
};

// The lanes of one device: made on demand, kept for the life of the process.  acquire() gives the lane with the fewest live
// sessions among the first max_lanes (the lowest index on a tie) and makes a new one -- make(Streams &) -> bool -- only when
// every existing one is taken and there is room.  Returns the lane's index, or -1 if `make` failed.
template <class Streams, class Member>
class LaneTable {
public:
    struct Lane {
        Streams streams{};
        int live = 0;
        LaneGather<Member> gather;
        RoundGather<Member> rounds;
    };
    template <class Make>
    int acquire(int max_lanes, Make &&make) {
        std::lock_guard<std::mutex> lock(m_);
        max_lanes = std::max(1, std::min(max_lanes, JTK_LANE_MAX_LANES));
        const int have = std::min<int>((int)lanes_.size(), max_lanes);
        int best = -1;
        for (int i = 0; i < have; i++)
            if (best < 0 || lanes_[i].live < lanes_[best].live) best = i;
        if ((best < 0 || lanes_[best].live > 0) && (int)lanes_.size() < max_lanes) {
            lanes_.emplace_back();
            if (!make(lanes_.back().streams)) {
                lanes_.pop_back();
                return -1;
            }
            best = (int)lanes_.size() - 1;
        }
        lanes_[best].live++;
        return best;
    }
    void release(int lane) {
        std::lock_guard<std::mutex> lock(m_);
        lanes_[lane].live--;
    }
    Lane &lane(int i) {  // (a deque: lanes never move)
        std::lock_guard<std::mutex> lock(m_);
        return lanes_[i];
    }
    int size() {
        std::lock_guard<std::mutex> lock(m_);
        return (int)lanes_.size();
    }
    int live(int i) {
        std::lock_guard<std::mutex> lock(m_);
        return lanes_[i].live;
    }

private:
    std::mutex m_;
    std::deque<Lane> lanes_;
};
