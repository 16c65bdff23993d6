"""The format keyword of every operator goes through one check (liquid_usrp_amd._format_code): a name of the table or a number equal
to one of its codes, anything else a ValueError that names the argument -- before any library call, so also on a machine without a
device.  No GPU."""
import pytest

BAD = ("sc8", "", "SC16", 2, -1)

CONSTRUCTORS = {
    "multichannelrx(input_format)": ("input_format", lambda p, v: p.multichannelrx(2, 64, 8, 4, input_format=v)),
    "multichanneltx(output_format)": ("output_format", lambda p, v: p.multichanneltx(2, 64, 8, 4, output_format=v)),
    "msresamp(input_format)": ("input_format", lambda p, v: p.msresamp(0.5, input_format=v)),
    "msresamp(output_format)": ("output_format", lambda p, v: p.msresamp(2.0, output_format=v)),
    "chanemu(output_format)": ("output_format", lambda p, v: p.chanemu(output_format=v)),
}


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
@pytest.mark.parametrize("ctor", sorted(CONSTRUCTORS))
def test_unknown_format_is_an_argument_error_without_a_device(product, ctor, bad):
    what, make = CONSTRUCTORS[ctor]
    with pytest.raises(ValueError) as ei:
        make(product, bad)
    assert what in str(ei.value)
    assert "cf32" in str(ei.value) and "sc16" in str(ei.value)          # the allowed names


def test_format_code_takes_names_and_equal_numbers(product):
    for table in (product.INPUT_FORMATS, product.OUTPUT_FORMATS):
        for name, code in table.items():
            assert product._format_code(name, table, "x") == code
            assert product._format_code(code, table, "x") == code and product._format_code(float(code), table, "x") == code
            assert type(product._format_code(float(code), table, "x")) is int
