"""What the tools that print per-kernel times share: the library's launch recorder (_lib.record_launches) over repeated calls."""
from musediffusion_amd import _lib


def timed(fn, calls, name=lambda kernel: kernel.split("(")[0]):
    """kernel name -> [microseconds] of the library launches fn makes, over `calls` calls.  `name`: kernel text as launched -> the name
    to print (default: up to the first parenthesis)"""
    def run():
        for _ in range(calls):
            fn()
    out = {}
    for r in _lib.record_launches(run):
        out.setdefault(name(r.kernel), []).append(1e3 * r.ms)
    return out
