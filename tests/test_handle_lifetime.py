"""A batch is destroyed through its context (gpet_batch_destroy waits on the context's stream), so whatever order the handles
are closed or finalised in, gpet_ctx_destroy must come after the gpet_batch_destroy of every batch built on that context.  Checked
on the CPU on the bookkeeping of _lib.Context / _lib.Batch with a recording stand-in for the library."""
import gc
import weakref


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def gpet_ctx_destroy(self, h):
        self.calls.append(("ctx", h))

    def gpet_batch_destroy(self, h):
        self.calls.append(("batch", h))


def _ctx(lib, h):
    from gaussian_process_edge_trace_amd import _lib
    c = _lib.Context.__new__(_lib.Context)
    c.lib, c.h, c._comms = lib, h, []
    c._batches, c._open_batches, c._close_pending = [], 0, False
    return c


def _batch(c, h):
    from gaussian_process_edge_trace_amd import _lib
    b = _lib.Batch.__new__(_lib.Batch)
    b.ctx, b.lib, b.h = c, c.lib, h
    c._batches.append(weakref.ref(b))
    c._open_batches += 1
    return b


def test_closing_a_context_closes_its_batches_first():
    lib = _Recorder()
    c = _ctx(lib, 1)
    a, b = _batch(c, 10), _batch(c, 11)
    a.close()
    c.close()  # (what a test's `finally: ctx.close()` does while a batch object is still a local)
    assert lib.calls == [("batch", 10), ("batch", 11), ("ctx", 1)]
    assert (a.h, b.h, c.h) == (None, None, None)
    b.close()
    c.close()
    del a, b, c
    gc.collect()
    assert len(lib.calls) == 3  # nothing is destroyed twice


def test_a_context_finalised_before_its_batches_is_destroyed_after_them():
    """The garbage collector clears weak references before it runs finalisers, and runs those in any order."""
    lib = _Recorder()
    c = _ctx(lib, 2)
    a, b = _batch(c, 20), _batch(c, 21)
    c._batches = []  # (dead weak references)
    c.__del__()
    assert lib.calls == [] and c.h == 2
    a.__del__()
    assert lib.calls == [("batch", 20)]
    b.__del__()
    assert lib.calls == [("batch", 20), ("batch", 21), ("ctx", 2)] and c.h is None


def test_batches_closed_first_leave_the_context_to_its_own_close():
    lib = _Recorder()
    c = _ctx(lib, 3)
    b = _batch(c, 30)
    b.close()
    assert lib.calls == [("batch", 30)] and c.h == 3
    c.close()
    assert lib.calls == [("batch", 30), ("ctx", 3)]
