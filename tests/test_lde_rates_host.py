"""The LDE size limits of the stage plan, without a device: qpgpu_stage_plan_create checks the header before it looks at the
context. An LDE of 2^21..2^23 points is accepted at any rate_bits (it used to need rate_bits <= 3); above 2^23 points the ceiling
and its message stay."""
import fri_schedules as fs
from test_stage_plan_host import create


def words_only(pkg, degree_bits, rate_bits):
    """The header-only words of the 24-wire synthetic circuit at 2^6 rows, restated as 2^degree_bits rows at rate_bits (the form
    without the constants/sigmas block does not grow with the row count)."""
    pack = pkg.synth_circuit(6, seed=63, num_wires=24, num_routed=16, num_public_inputs=3)[0]
    arity = fs.constant_arity(degree_bits, rate_bits, 4, 4, 5)
    w = fs.with_schedule(pkg.stage_header_words(pack), arity, rate_bits=rate_bits, cap_height=4)
    w[1] = degree_bits
    assert pkg.pack_header(w)["degree_bits"] == degree_bits and pkg.pack_header(w)["rate_bits"] == rate_bits
    return w


def test_rate_5_at_2p16_rows_passes_the_header_check(pkg):
    rc, msg = create(pkg, words_only(pkg, 16, 5))
    assert "rate_bits <= 3" not in msg
    assert (rc, msg) == (-1, "stage_plan_create: null context")


def test_every_rate_up_to_2p23_points(pkg):
    for d, r in ((13, 8), (14, 7), (15, 8), (16, 7), (19, 4), (20, 3)):
        assert create(pkg, words_only(pkg, d, r)) == (-1, "stage_plan_create: null context"), (d, r)


def test_the_2p23_ceiling_stays(pkg):
    assert create(pkg, words_only(pkg, 16, 8)) == (-1, "stage_plan_create: LDE larger than 2^23 not supported")
    assert create(pkg, words_only(pkg, 20, 4)) == (-1, "stage_plan_create: LDE larger than 2^23 not supported")
