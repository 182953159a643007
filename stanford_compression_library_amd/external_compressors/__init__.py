"""Wrappers around codecs that live outside this package, by the reference's module names (pickle only)."""
