"""What the CPU tests of the C entry points share: a refusal is code 1 and the entry point's own message, before any launch."""
from makani_amd import _lib

A = 4096      # a non-null, 16-byte aligned address that is never dereferenced: validation returns before any launch


def case_ids(cases):
    """`entry point-words of the message-position in the table`: readable, unique and the same in every run."""
    return [f"{c[0]}-{'_'.join(c[2].split()[:2])}-{i}" for i, c in enumerate(cases)]


def assert_refused(name, args, msg, who=None):
    """``name(*args, stream)`` returns 1 and leaves ``who: msg`` (``who``: the function the check lives in, default ``name``)."""
    lib = _lib.load()
    lib.mk_quadrature(7, 10, 0, 0)      # leaves a message of another function behind: the one below must replace it
    assert getattr(lib, name)(*args, None) == 1
    assert lib.mk_last_error() == f"{who or name}: {msg}".encode()
