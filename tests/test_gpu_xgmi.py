"""libmi355x_xgmi.so on an MI355X: the kernel-driven xGMI test with device 0 as its own peer -- the kernel, its
slicing of the workgroups among the destinations, the verification and its self-check are what a one-GPU box can
exercise (its rates are local-HBM rates, not link rates: none is asserted).  With a second GPU the matrix runs too."""
import pytest

pytestmark = pytest.mark.gpu

RAGGED = (1 << 20) + 16 * 37
# a single element, less than one workgroup's 32 KiB chunk, a ragged tail behind 32 full chunks
SIZES = (16, 4096 + 16, RAGGED)


@pytest.fixture(scope="module")
def xgmi():
    from k8s_gpu_node_checker_amd.ops import xgmi as x
    assert x.device_count() >= 1
    return x


def _clean(r, ndst, mode):
    assert r["src"] == 0 and r["mode"] == mode and len(r["to"]) == ndst and not r.get("hung")
    for t in r["to"]:
        assert t["dst"] == 0 and t["errors"] == 0 and t["first_bad"] is None and t["peer"] is True, t
        assert t["gbps"] > 0, t
    assert r["total_gbps"] > 0
    # each destination's window lies inside the events' window, so the per-destination rates add up to the total
    # or more; the factor of 0.5 leaves room for the two clocks (the wall clock's 10 ns ticks, the events')
    assert sum(t["gbps"] for t in r["to"]) >= 0.5 * r["total_gbps"], r


@pytest.mark.parametrize("mode", ("store", "load"))
@pytest.mark.parametrize("ndst", (1, 3, 7))
def test_clean_runs(xgmi, mode, ndst):
    for iters in (1, 2):
        for nbytes in SIZES:
            r = xgmi.kernel_fan(0, [0] * ndst, iters=iters, mode=mode, nbytes=nbytes)
            print(mode, ndst, iters, nbytes, r)
            _clean(r, ndst, mode)


@pytest.mark.parametrize("mode", ("store", "load"))
@pytest.mark.parametrize("word", (RAGGED // 4 - 1, 0))
def test_injected_fault_is_found_in_its_destination_only(xgmi, mode, word):
    iters = 2
    r = xgmi.kernel_fan(0, [0, 0, 0], iters=iters, mode=mode, nbytes=RAGGED, inject_dst=1, inject_word=word)
    print(mode, word, r)
    hit, others = r["to"][1], (r["to"][0], r["to"][2])
    assert hit["errors"] == (1 if mode == "store" else iters) and hit["first_bad"] == word // 4, r
    assert all(t["errors"] == 0 and t["first_bad"] is None for t in others), r


def test_rejections_are_raised(xgmi):
    n = xgmi.device_count()
    for kw in (dict(src=n, dsts=[0]), dict(src=-1, dsts=[0]), dict(src=0, dsts=[n]), dict(src=0, dsts=[0, -1]),
               dict(src=0, dsts=[]), dict(src=0, dsts=[0] * 65), dict(src=0, dsts=[0], nbytes=8),
               dict(src=0, dsts=[0], nbytes=4096, inject_dst=0, inject_word=1024),
               dict(src=0, dsts=[0], nbytes=4096, inject_dst=0, inject_word=-1),
               dict(src=0, dsts=[0], nbytes=4096, inject_dst=1, inject_word=0)):
        kw.setdefault("nbytes", 4096)
        with pytest.raises(RuntimeError, match=r"xgmi failed \(-2\)"):
            xgmi.kernel_fan(iters=1, **kw)
    with pytest.raises(ValueError):
        xgmi.kernel_fan(0, [0], nbytes=4096, mode="copy")
    # nothing above left the device in an error state
    _clean(xgmi.kernel_fan(0, [0], iters=1, nbytes=4096), 1, "store")


@pytest.mark.parametrize("mode", ("store", "load"))
def test_with_a_deadline_the_result_is_the_same(xgmi, mode):
    r = xgmi.kernel_fan(0, [0, 0, 0], iters=2, mode=mode, nbytes=RAGGED, timeout_s=30)
    _clean(r, 3, mode)
    hit = xgmi.kernel_fan(0, [0, 0, 0], iters=2, mode=mode, nbytes=RAGGED, timeout_s=30, inject_dst=2, inject_word=5)
    assert [t["errors"] for t in hit["to"]] == [0, 0, 1 if mode == "store" else 2] and hit["to"][2]["first_bad"] == 1


def test_matrix(xgmi):
    assert "skipped" in xgmi.kernel_matrix([0])
    if xgmi.device_count() < 2:
        return  # one GPU: no pair to run (the self-peer tests above are what this box can show)
    from k8s_gpu_node_checker_amd.ops import diag
    m = xgmi.kernel_matrix([0, 1], mib=64, iters=2)
    print(m)
    assert len(m["pairs"]) == 4 and len(m["fan"]) == 4 and m["bad"] == [] and "stopped" not in m and "failed" not in m
    assert all(r["errors"] == 0 and r["peer"] for r in m["pairs"] + m["fan"])
    p = diag.p2p_matrix([0, 1], mib=64, iters=2, kernel=True)
    print(p)
    assert p["pass"], p["detail"]
