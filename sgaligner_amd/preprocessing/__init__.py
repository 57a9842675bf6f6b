"""Preprocessing steps of the reference's preprocessing/scan3r package that run on the device (subscans.py: subscan generation)."""
