// powell_batch.h -- many independent Powell searches advanced in lockstep: each problem runs the unchanged powellOptimizer of powell.h
// inside a stackful coroutine (glibc makecontext / swapcontext, a private stack each) that pauses at every cost call; the scheduler
// collects one parameter vector from each live search, hands all of them to a batch cost callback in one call, and resumes the searches
// with their costs. A finished search gives its slot to the next problem. One code path for the search: a problem's sequence of cost
// calls, and so its result, is exactly what powellOptimizer does alone, whatever shares its batch.
// The coroutines do host arithmetic only; the callback (where a device is used) always runs on the scheduler's own stack.
// Host only; no device code.
#ifndef XH_POWELL_BATCH_H
#define XH_POWELL_BATCH_H
#include <ucontext.h>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "powell.h"

namespace xh_powell {

// cost of m rows: row r is problem[r] with its variables at x[r * nmax .. r * nmax + n - 1] (0-based); returns 0, or an error code that
// ends the whole run
typedef int32_t (*BatchCostFn)(int32_t m, const int32_t *problem, const double *x, double *cost, void *user);
// optional: a cost the host can decide without the batch callback (a bound check). Returns 1 and sets *cost if it did.
typedef int32_t (*PreCostFn)(int32_t problem, const double *x, double *cost, void *user);

struct Lockstep {
    struct Abort {};
    struct Slot {
        Lockstep *owner;
        ucontext_t co;
        int problem, n;
        std::vector<double> p, steps;
        double cost, fret;
        int iter;
        int64_t evals;
        bool waiting, done;
        double *x;          // this slot's row of the batch
    };
    // Contract of the stacks: they are one block without guard pages. What runs on a search's stack is powellOptimizer (its arrays are on
    // the heap), cost_tramp and `pre`, which must stay small (today a bound check of a few hundred bytes); `f` runs on the scheduler's stack.
    // A pause and a resume are two swapcontext calls, each with a sigprocmask system call.
    static const size_t kStack = 64 * 1024;
    static const int kNoStacks = 0x7fffffff;

    int nmax;
    double ftol;
    PreCostFn pre;
    void *user;
    bool aborting;
    ucontext_t sched;
    std::vector<Slot> slots;
    std::vector<double> rows;
    char *stacks;

    Lockstep() : aborting(false), stacks(nullptr) {}
    ~Lockstep() { std::free(stacks); }

    static double cost_tramp(double *x, void *prm)
    {
        Slot *s = (Slot *)prm;
        Lockstep *L = s->owner;
        ++s->evals;
        for (int j = 0; j < s->n; ++j) s->x[j] = x[1 + j];
        double c;
        if (L->pre && L->pre(s->problem, s->x, &c, L->user)) return c;
        s->waiting = true;
        swapcontext(&s->co, &L->sched);
        s->waiting = false;
        if (L->aborting) throw Abort();
        return s->cost;
    }

    static void entry(unsigned lo, unsigned hi)
    {
        Slot *s = (Slot *)(((uintptr_t)hi << 32) | (uintptr_t)lo);
        try {
            powellOptimizer(s->p, 1, s->n, cost_tramp, s, s->owner->ftol, s->fret, s->iter, s->steps);
        } catch (const Abort &) {
        }
        s->done = true;     // returning resumes uc_link, the scheduler
    }

    // starts `problem` in slot k and runs it to its first pause (or to its end, when the host decides every cost)
    void start(int k, int problem, int n, const double *p, const double *steps)
    {
        Slot &s = slots[k];
        s.problem = problem; s.n = n;
        s.p.assign(p, p + n);
        s.steps.assign(steps, steps + n);
        s.evals = 0; s.iter = 0; s.fret = 0; s.waiting = false; s.done = false;
        getcontext(&s.co);
        s.co.uc_stack.ss_sp = stacks + (size_t)k * kStack;
        s.co.uc_stack.ss_size = kStack;
        s.co.uc_link = &sched;
        const uintptr_t a = (uintptr_t)&s;
        makecontext(&s.co, (void (*)())entry, 2, (unsigned)(a & 0xffffffffu), (unsigned)(a >> 32));
        swapcontext(&sched, &s.co);
    }

    // p, steps: [nprob][nmax]; fret, iter, evals: [nprob] (evals nullable). Returns 0, kNoStacks or the callback's error.
    int run(int nprob, const int32_t *n, int nmax_, double *p, const double *steps, double ftol_, int capacity, BatchCostFn f, PreCostFn pre_,
            void *user_, double *fret, int32_t *iter, int64_t *evals)
    {
        nmax = nmax_; ftol = ftol_; pre = pre_; user = user_;
        const int cap = std::max(1, std::min(capacity, nprob));
        stacks = (char *)std::malloc((size_t)cap * kStack);
        if (!stacks) return kNoStacks;
        slots.resize((size_t)cap);
        rows.assign((size_t)cap * nmax, 0.0);
        std::vector<int32_t> idx((size_t)cap), who((size_t)cap);
        std::vector<double> xs((size_t)cap * nmax), cs((size_t)cap);
        std::vector<char> live((size_t)cap, 0);
        for (int k = 0; k < cap; ++k) { slots[k].owner = this; slots[k].x = &rows[(size_t)k * nmax]; }
        int next = 0, rc = 0;
        auto retire = [&](int k) {
            Slot &s = slots[k];
            for (int j = 0; j < s.n; ++j) p[(size_t)s.problem * nmax + j] = s.p[j];
            fret[s.problem] = s.fret;
            iter[s.problem] = s.iter;
            if (evals) evals[s.problem] = s.evals;
            live[k] = 0;
        };
        auto refill = [&](int k) {
            while (!live[k] && next < nprob) {
                const int q = next++;
                live[k] = 1;
                start(k, q, n[q], p + (size_t)q * nmax, steps + (size_t)q * nmax);
                if (slots[k].done) retire(k);
            }
        };
        for (int k = 0; k < cap; ++k) refill(k);
        for (;;) {
            int m = 0;
            for (int k = 0; k < cap; ++k)
                if (live[k]) {
                    who[m] = k;
                    idx[m] = slots[k].problem;
                    for (int j = 0; j < nmax; ++j) xs[(size_t)m * nmax + j] = j < slots[k].n ? slots[k].x[j] : 0.0;
                    ++m;
                }
            if (m == 0) break;
            if (!aborting) {
                rc = f(m, idx.data(), xs.data(), cs.data(), user);
                if (rc != 0) aborting = true;      // every paused search is unwound by an exception on its own stack
            }
            for (int r = 0; r < m; ++r) {
                const int k = who[r];
                slots[k].cost = cs[r];
                swapcontext(&sched, &slots[k].co);
                if (slots[k].done) {
                    if (aborting) live[k] = 0;
                    else { retire(k); refill(k); }
                }
            }
            if (aborting) break;
        }
        return rc;
    }
};

}  // namespace xh_powell
#endif
