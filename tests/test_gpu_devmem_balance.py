"""GPU: what the library takes from the driver it gives back.  A fresh process (tests/devmem_balance_child.py) runs scan, count, EC graph, correction, assembly
graph and read alignment on 64 reads, assembles one batch from two handles, and closes every handle, with the allocation log on and no pool: the sizes on the
successful hipMalloc lines are, as a multiset, the sizes on the hipFree lines.  (The buffers free themselves -- csrc/devmem.hpp, ~DevBuf --, no list of them
is kept anywhere: this is the test that a struct's buffer cannot be forgotten.)"""
import collections
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_hipmalloc_is_freed_by_destroy():
    env = {k: v for k, v in os.environ.items() if k not in ("OATK_TEST_POOL", "OATK_DEBUG_POOL_MIN", "OATK_DEBUG_POOL_SEQ")}
    env.update(OATK_DEBUG_ALLOC_LOG="1", OATK_POOL="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "devmem_balance_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "closed: 64 reads" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    took = collections.Counter(re.findall(r"\[oatk alloc\] [\d.]+ hipMalloc +([\d.]+) MB: [\d.]+ s$", p.stderr, re.M))
    gave = collections.Counter(re.findall(r"\[oatk alloc\] [\d.]+ hipFree +([\d.]+) MB: [\d.]+ s$", p.stderr, re.M))
    print("%d hipMalloc, %d hipFree, %d sizes" % (sum(took.values()), sum(gave.values()), len(took)))
    assert sum(took.values()) >= 50, "the log does not show the pipeline's buffers"            # (the handle alone has 50, before any state struct)
    assert " pieces " not in p.stderr and "FAILED" not in p.stderr
    assert took == gave, {"held after destroy": took - gave, "freed but never taken": gave - took}
