"""The stencil builder and the launch-group walk of the differenced gradients (csrc/grad_stencil.inc, over csrc/api_kparams.inc) on the
host (no GPU): csrc/test_aids/grad_stencil_host.cpp is a stand-alone program, compiled from the two files with the address and
undefined-behaviour sanitizers, that runs a stencil without entries, 11 entries of one product term (two launch groups, 8 + 3) and
interleaved entries of a three-term model through both, checks the launch order, the offsets, the groups and the stencil points'
parameters, and the refusals with their status and text: a term out of range, a step of 0, a step of inf, a Matern order the fit
refuses."""
import os
import subprocess


def test_stencils_through_the_builder_and_the_group_walk():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "grad_stencil_host"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(here, "build", "grad_stencil_host")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:]
