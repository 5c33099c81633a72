"""The order table of the large GEMM launches (csrc/tile_order.hpp) on the host (no GPU): csrc/test_aids/tile_order_host.cpp is a
stand-alone program, compiled from the header with the address and undefined-behaviour sanitizers, that sweeps launches of 8, 33, 36,
82 and 124 tile rows and columns, live-row limits that cut zero, one and two tile rows, and 0, 4 and 6 urgent columns, and checks
that every needed tile appears exactly once, none starts at or beyond the limit, the urgent tiles come first in every XCD's list, the
lists are balanced, and with the limit at "all rows" the table is the one the builder made before it took a limit (a verbatim copy
of that loop is the reference).  Balance: the lists differ by at most one tile without urgent columns; with urgent columns the urgent
tiles and the rest are two sequences, each cut evenly with its remainder on the first XCDs, so each part differs by at most one and
the whole lists by at most two (27 of the sweep's 30 urgent cases do differ by two) -- the old table does the same."""
import os
import subprocess


def test_order_table_properties_and_the_old_table():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "tile_order_host"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(here, "build", "tile_order_host")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 5 * 3 * 3, r.stdout[-4000:]
