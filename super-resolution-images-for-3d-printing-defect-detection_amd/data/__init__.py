"""The reference's data/ folder: the exploratory data analysis (eda_methods)."""
