"""A captured graph holds what it reads.

A hipGraph bakes raw device and pinned-host addresses into its nodes.  future_od/graph.py opens a `Record` around each
capture it makes and keeps it in the graph's own dict, so the memory lives exactly as long as the graph can be replayed;
a producer that replaces or drops something simply lets go of it.

  * `hold(kind, obj)` at a site that hands an address of memory it may later replace to a launch: one global test,
    nothing else, when no record is open.
  * `provide(fn)`: state that every capture uses and that is touched hundreds of times per step (the prepared-operand
    store, the gradient arena) is not held per use; the record asks `fn() -> [(kind, obj), ...]` once, when it closes.
  * `hold_or_ask(kind, obj)` for sites that are rare or already know that the stream is capturing: a capture that
    graph.py did not open ("foreign": someone's own torch.cuda.graph) has no record, so the object -- and what the
    providers name at that moment -- goes to `FOREIGN` for the life of the process.  A foreign capture is noticed
    only at these sites.

A record does nothing at replay time; `of(kind)` tells a test or a person what a graph holds."""
import torch

_open = None            # the record of the capture in progress
_providers = []
FOREIGN = {}            # id -> (kind, obj): the only keep-alive list outside graph records


def _collect(into):
    for fn in _providers:
        for kind, obj in fn():
            if obj is not None:
                into[id(obj)] = (kind, obj)


class Record:
    def __init__(self):
        self.held = {}          # id -> (kind, obj): strong references, one per object

    def __enter__(self):
        global _open
        assert _open is None, "capture records do not nest"
        _open = self
        return self

    def __exit__(self, *exc):
        global _open
        _open = None
        _collect(self.held)

    def of(self, kind):
        return [obj for k, obj in self.held.values() if k == kind]


def provide(fn):
    _providers.append(fn)


def hold(kind, obj):
    if _open is not None:
        _open.held[id(obj)] = (kind, obj)


def hold_or_ask(kind, obj):
    """True if `obj` is now held (a capture is in progress)."""
    if _open is not None:
        _open.held[id(obj)] = (kind, obj)
    elif torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
        FOREIGN[id(obj)] = (kind, obj)
        _collect(FOREIGN)
    else:
        return False
    return True
