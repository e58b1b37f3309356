"""The reference of the transports with per-cell layer thicknesses (nf_field_set_cell_thickness): tests/resolved_reference.py
with the thickness read at the face.  That module defines the terms, fixed(.) of e3u / e3v included, and the summation."""
from resolved_reference import ResolvedReference, array_values  # noqa: F401  (array_values: for the callers)


class CellThickReference(ResolvedReference):
    """ResolvedReference with cell_thickness=True.  thick_markers: the markers of e3u / e3v (NaN = unused)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **dict(kw, cell_thickness=True))
