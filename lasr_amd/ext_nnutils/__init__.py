"""Restated networks of the reference's third_party/ext_nnutils used by the preprocessing scripts."""
