/*
 * The queue of deferred transfer callbacks (libplacebo_amd/csrc/host/cbq.h) on its own, without a
 * device: a fence here is a heap-allocated "time at which it completes", asked against a clock
 * the test turns, and freed when the queue releases it -- so a fence touched after its release,
 * or an entry read after it was taken out, is a heap-use-after-free under AddressSanitizer
 * (tests/c/cbq_sanitize.mk builds and runs this file with -fsanitize=address,undefined;
 * tests/test_callback_queue.py builds it plain and checks the same expectations).
 *
 * Checked: callbacks run in the order they were queued, each exactly once, none before its fence
 * has completed (an older, unfinished entry holds back younger finished ones); a callback may
 * queue more work and reach a drain point itself; 80 entries pass through the capacity of 64.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cbq.h"

static int g_now;               // the clock
static int g_released, g_waits;
static int g_order[256], g_ran; // ids in the order their callbacks ran
static int g_failed;

#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); g_failed = 1; } } while (0)

static bool f_done(void *ctx, void *fence)  { (void) ctx; return *(int *) fence <= g_now; }
static void f_wait(void *ctx, void *fence)  { (void) ctx; g_waits++; if (*(int *) fence > g_now) g_now = *(int *) fence; }
static void f_release(void *ctx, void *fence) { (void) ctx; g_released++; free(fence); }

static void *fence_at(int t)
{
    int *f = malloc(sizeof(*f));
    *f = t;
    return f;
}

static struct plh_cbq *queue_new(void)
{
    struct plh_cbq *q = calloc(1, sizeof(*q));
    q->done = f_done;
    q->wait = f_wait;
    q->release = f_release;
    g_now = g_released = g_waits = g_ran = 0;
    memset(g_order, 0, sizeof(g_order));
    return q;
}

struct item { int id; int due; struct plh_cbq *q; struct item *spawn; };

static void cb_plain(void *priv)
{
    struct item *it = priv;
    CHECK(it->due <= g_now);            // never before its fence
    g_order[g_ran++] = it->id;
}

// a callback that starts another transfer and then reaches a drain point, as pl_tex_upload would
static void cb_reenter(void *priv)
{
    struct item *it = priv;
    CHECK(it->due <= g_now);
    g_order[g_ran++] = it->id;
    if (it->spawn) {
        plh_cbq_push(it->q, fence_at(it->spawn->due), cb_plain, it->spawn);
        plh_cbq_drain(it->q, false);
    }
}

static void expect_order(const int *want, int n)
{
    CHECK(g_ran == n);
    for (int i = 0; i < n && i < g_ran; i++)
        CHECK(g_order[i] == want[i]);
}

static void test_order_and_once(void)
{
    struct plh_cbq *q = queue_new();
    struct item it[10];
    for (int i = 0; i < 10; i++) {
        it[i] = (struct item) { .id = i, .due = i + 1 };
        plh_cbq_push(q, fence_at(i + 1), cb_plain, &it[i]);
    }
    plh_cbq_drain(q, false);
    CHECK(g_ran == 0 && q->count == 10);
    g_now = 3;
    plh_cbq_drain(q, false);
    CHECK(g_ran == 3 && q->count == 7);
    plh_cbq_drain(q, false);            // nothing twice
    CHECK(g_ran == 3);
    g_now = 10;
    plh_cbq_drain(q, false);
    const int want[10] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9 };
    expect_order(want, 10);
    CHECK(q->count == 0 && g_released == 10 && g_waits == 0);
    free(q);
}

static void test_older_entry_holds_back_younger(void)
{
    struct plh_cbq *q = queue_new();
    struct item it[3] = { { .id = 0, .due = 5 }, { .id = 1, .due = 1 }, { .id = 2, .due = 2 } };
    for (int i = 0; i < 3; i++)
        plh_cbq_push(q, fence_at(it[i].due), cb_plain, &it[i]);
    g_now = 2;
    plh_cbq_drain(q, false);
    CHECK(g_ran == 0);
    g_now = 5;
    plh_cbq_drain(q, false);
    const int want[3] = { 0, 1, 2 };
    expect_order(want, 3);
    free(q);
}

static void test_reentry(void)
{
    struct plh_cbq *q = queue_new();
    struct item spawned = { .id = 100, .due = 1 };     // already complete when it is queued
    struct item late = { .id = 101, .due = 50 };
    struct item it[3] = {
        { .id = 0, .due = 1, .q = q, .spawn = &spawned },
        { .id = 1, .due = 2, .q = q, .spawn = &late },
        { .id = 2, .due = 3, .q = q },
    };
    for (int i = 0; i < 3; i++)
        plh_cbq_push(q, fence_at(it[i].due), cb_reenter, &it[i]);
    g_now = 3;
    plh_cbq_drain(q, false);
    // 0 runs, queues 100 behind 2 and drains: 1 (queues 101, drains: 2, 100), back in 0, back out
    const int want[4] = { 0, 1, 2, 100 };
    expect_order(want, 4);
    CHECK(q->count == 1);
    plh_cbq_drain(q, true);             // waits for 101
    CHECK(g_ran == 5 && g_order[4] == 101 && q->count == 0 && g_now == 50 && g_waits == 1);
    CHECK(g_released == 5);
    free(q);
}

static void test_eighty_through_sixty_four(void)
{
    struct plh_cbq *q = queue_new();
    static struct item it[80];
    for (int i = 0; i < 80; i++) {
        it[i] = (struct item) { .id = i, .due = 1000 + i };
        plh_cbq_push(q, fence_at(it[i].due), cb_plain, &it[i]);
        CHECK(q->count <= PLH_CBQ_CAP);
    }
    // the 65th .. 80th push each waited for the oldest entry and ran it
    CHECK(g_ran == 80 - PLH_CBQ_CAP && q->count == PLH_CBQ_CAP && g_waits == 80 - PLH_CBQ_CAP);
    plh_cbq_drain(q, false);
    CHECK(g_ran == 80 - PLH_CBQ_CAP);   // the clock stands where the last wait left it
    plh_cbq_drain(q, true);
    CHECK(g_ran == 80 && q->count == 0 && g_released == 80);
    for (int i = 0; i < 80; i++)
        CHECK(g_order[i] == i);
    free(q);
}

// a full queue, and the callback the push has to run first queues an entry of its own
static void test_push_from_callback_of_a_full_queue(void)
{
    struct plh_cbq *q = queue_new();
    static struct item it[PLH_CBQ_CAP + 1];
    struct item spawned = { .id = 200, .due = 1 };
    for (int i = 0; i < PLH_CBQ_CAP; i++) {
        it[i] = (struct item) { .id = i, .due = 10 + i, .q = q, .spawn = i == 0 ? &spawned : NULL };
        plh_cbq_push(q, fence_at(it[i].due), cb_reenter, &it[i]);
    }
    it[PLH_CBQ_CAP] = (struct item) { .id = PLH_CBQ_CAP, .due = 500 };
    plh_cbq_push(q, fence_at(500), cb_plain, &it[PLH_CBQ_CAP]);
    CHECK(q->count <= PLH_CBQ_CAP);
    plh_cbq_drain(q, true);
    CHECK(q->count == 0 && g_ran == PLH_CBQ_CAP + 2 && g_released == PLH_CBQ_CAP + 2);
    // everything once; 200 was queued before the entry whose push made room for it
    int seen[PLH_CBQ_CAP + 2] = {0}, pos200 = -1, pos_last = -1;
    for (int i = 0; i < g_ran; i++) {
        const int id = g_order[i] == 200 ? PLH_CBQ_CAP + 1 : g_order[i];
        seen[id]++;
        if (g_order[i] == 200) pos200 = i;
        if (g_order[i] == PLH_CBQ_CAP) pos_last = i;
    }
    for (int i = 0; i < PLH_CBQ_CAP + 2; i++)
        CHECK(seen[i] == 1);
    CHECK(pos200 >= 0 && pos200 < pos_last);
    free(q);
}

int main(void)
{
    test_order_and_once();
    test_older_entry_holds_back_younger();
    test_reentry();
    test_eighty_through_sixty_four();
    test_push_from_callback_of_a_full_queue();
    if (g_failed)
        return 1;
    printf("ok\n");
    return 0;
}
