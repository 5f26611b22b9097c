"""Run a rate tool unchanged and append, to every line it prints, the minor page faults its latest timed loop took (the two latest
time.perf_counter() calls bracket it): host paths that allocate their output arrays per step pay for the pages glibc hands back to the
system and faults in again.  usage: python tools/page_faults.py tools/host_path_rate.py
(with MALLOC_TRIM_THRESHOLD_=1073741824 MALLOC_MMAP_THRESHOLD_=33554432 in the environment glibc keeps the pages)"""
import builtins
import resource
import runpy
import sys
import time

real_clock, real_print, seen = time.perf_counter, builtins.print, [0, 0]


def clock():
    seen.append(resource.getrusage(resource.RUSAGE_SELF).ru_minflt)
    return real_clock()


def show(*args, **kw):
    real_print(*args, f" | minor page faults in the timed loop: {seen[-1] - seen[-2]}", **kw)


time.perf_counter, builtins.print = clock, show
sys.argv = sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
