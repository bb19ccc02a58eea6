/*
 * libplacebo-hip -- the queue of deferred transfer callbacks (pl_tex_transfer_params.callback).
 * A transfer that carries a callback records a fence behind its last operation and pushes
 * { fence, fn, priv } here; the entries are run in order, each once its fence has completed, from
 * the calling thread at the points gpu_hip.c names. Pure host code: what a fence is and how it is
 * asked is the owner's business (gpu_hip.c: an event of the fence pool; tests/c/cbq_sanitize.c: a
 * counter), so the queue runs without a device.
 *
 * An entry is taken out BEFORE its function is called: the function may start transfers (push)
 * and reach a drain point itself.
 */
#ifndef PLH_CBQ_H_
#define PLH_CBQ_H_

#include <stdbool.h>
#include <stddef.h>

#define PLH_CBQ_CAP 64

struct plh_cbq_entry {
    void *fence;
    void (*fn)(void *priv);
    void *priv;
};

struct plh_cbq {
    struct plh_cbq_entry e[PLH_CBQ_CAP];
    unsigned head, count;   // e[head] is the oldest entry
    void *ctx;
    bool (*done)(void *ctx, void *fence);       // has the fence completed? (never blocks)
    void (*wait)(void *ctx, void *fence);       // returns once it has
    void (*release)(void *ctx, void *fence);    // the (completed) fence is no longer needed
};

static inline void plh_cbq_run_oldest(struct plh_cbq *q)
{
    const struct plh_cbq_entry e = q->e[q->head];
    q->head = (q->head + 1) % PLH_CBQ_CAP;
    q->count--;
    q->release(q->ctx, e.fence);
    e.fn(e.priv);
}

// Runs, oldest first, every entry whose fence has completed and stops at the first that has not;
// with `all` it waits for that one instead, so the queue is empty afterwards -- including what
// the functions themselves pushed meanwhile.
static inline void plh_cbq_drain(struct plh_cbq *q, bool all)
{
    while (q->count) {
        void *fence = q->e[q->head].fence;
        if (!q->done(q->ctx, fence)) {
            if (!all)
                return;
            q->wait(q->ctx, fence);
        }
        plh_cbq_run_oldest(q);
    }
}

// Takes over `fence`. With the queue full the oldest entry is waited for and run first.
static inline void plh_cbq_push(struct plh_cbq *q, void *fence, void (*fn)(void *priv), void *priv)
{
    while (q->count == PLH_CBQ_CAP) {
        q->wait(q->ctx, q->e[q->head].fence);
        plh_cbq_run_oldest(q);
    }
    q->e[(q->head + q->count) % PLH_CBQ_CAP] = (struct plh_cbq_entry) { fence, fn, priv };
    q->count++;
}

#endif // PLH_CBQ_H_
