"""Drop-in for the reference's compressors.py."""
from _mx_pkg import PKG

get_top_k = PKG.get_top_k
get_scaled_sign = PKG.get_scaled_sign
unpack_scaled_sign = PKG.unpack_scaled_sign
